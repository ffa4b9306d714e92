"""CPU tier: what CraftingWorldVecEnv.replay_push / replay_sample / replay_clear hand to the library -- entry point, scalars, which pointer sits in which
slot, the NULL members of fields not named, the seed forms, the rounding of `her`, that no call synchronises, and what raises before any call
(tests/recording_engine.py: the env without an engine, a library that takes notes), after tests/test_refit_calls.py."""
import numpy as np
import pytest
import torch

from gym_craftingworld_amd import _lib as L
from gym_craftingworld_amd.vec_env import REPLAY_FIELDS
from recording_engine import make_env, release
from test_vec_env_calls import N, S, at, raises_before_any_call, the_call

B = 7
DTYPES = dict(hdr=torch.uint8, slot_pos=torch.int16, next_hdr=torch.uint8, next_slot_pos=torch.int16, goal_hdr=torch.uint8, goal_slot_pos=torch.int16,
              action=torch.uint8, reward=torch.int32, done=torch.bool, desired=torch.int16, env=torch.int32, slot=torch.int32, future=torch.int32)


@pytest.fixture(params=[False, True], ids=['device_outputs', 'host_outputs'])
def env(request):
    e = make_env(N, S, host_outputs=request.param)
    e._host_actions = np.full(N, 99, np.int32)               # (the engine's mapped action buffer, as the constructor views it)
    yield e
    release(e)


def shapes(b, names=REPLAY_FIELDS):
    return {f: ((b, 16) if f.endswith('hdr') else (b, 8) if f.endswith('slot_pos') else (b,), DTYPES[f]) for f in names}


def check_out(out, want, struct):
    """the returned dict against the spec, and the struct the library got: a field's member holds its tensor's pointer, every other member is NULL"""
    assert list(out) == list(want) and {f: (tuple(t.shape), t.dtype) for f, t in out.items()} == want
    assert list(struct) == list(REPLAY_FIELDS)
    for f in REPLAY_FIELDS:
        assert struct[f] == (out[f].data_ptr() if f in out else None), f


def test_replay_sample(env):
    r = env.replay_sample(B)
    b, seed, seed_dev, her, strategy, struct = the_call(env, 'cw_replay_sample', sync=False)      # (nothing a host reads next: no synchronisation)
    assert (b, seed, seed_dev, her, strategy) == (B, 0, None, 0, 0)
    check_out(r, shapes(B), struct)                                # the default: all thirteen
    assert env.replay_sample(B, 5, out=r) is r                     # an earlier call's dict, written again
    args = the_call(env, 'cw_replay_sample', sync=False)
    assert args[1] == 5
    check_out(r, shapes(B), args[-1])
    env.replay_sample(np.int64(B), 2 ** 64 - 1, her=1.0, strategy='final')
    b, seed, seed_dev, her, strategy, struct = the_call(env, 'cw_replay_sample', sync=False)
    assert (b, seed, seed_dev, her, strategy) == (B, 2 ** 64 - 1, None, 65536, 1)
    assert all(at(env, p) is not None for p in struct.values())    # kept alive: the kernel may not have run yet


def test_fields_not_named_are_null(env):
    r = env.replay_sample(B, fields=('reward',))
    struct = the_call(env, 'cw_replay_sample', sync=False)[-1]
    check_out(r, shapes(B, ('reward',)), struct)
    assert [f for f, v in struct.items() if v is not None] == ['reward']
    r = env.replay_sample(B, fields=('goal_hdr', 'hdr', 'future'))
    struct = the_call(env, 'cw_replay_sample', sync=False)[-1]
    check_out(r, shapes(B, ('goal_hdr', 'hdr', 'future')), struct)
    assert sorted(f for f, v in struct.items() if v is not None) == ['future', 'goal_hdr', 'hdr']


@pytest.mark.parametrize('her, word', [(0.0, 0), (1.0, 65536), (0.5, 32768), (0.8, 52429), (1 / 65536, 1), (0.4 / 65536, 0), (0.6 / 65536, 1), (1, 65536), (0, 0),
                                       (np.float32(0.25), 16384), (1 - 0.4 / 65536, 65536)])
def test_her_goes_over_as_round_her_times_65536(env, her, word):
    env.replay_sample(B, her=her)
    assert the_call(env, 'cw_replay_sample', sync=False)[3] == word


@pytest.mark.parametrize('dtype', [torch.int64, torch.uint64])
def test_the_seed_as_a_tensor_goes_over_as_the_device_word(env, dtype):
    word = torch.tensor([41], dtype=dtype)
    env.replay_sample(B, word)
    args = the_call(env, 'cw_replay_sample', sync=False)
    assert args[1] == 0 and args[2] == word.data_ptr()
    del word
    assert at(env, args[2]).tolist() == [41]                       # kept alive: a captured graph reads it on every replay
    word = torch.tensor([3], dtype=dtype)
    env.replay_sample(B, (9, word))                                # both at once: the kernel adds them
    args = the_call(env, 'cw_replay_sample', sync=False)
    assert args[1] == 9 and args[2] == word.data_ptr()


def test_an_empty_batch_makes_no_call(env):
    r = env.replay_sample(0)
    assert env._lib.calls == [] and {f: tuple(t.shape) for f, t in r.items()} == {f: s for f, (s, _) in shapes(0).items()}


def test_what_raises_before_any_call(env):
    r = env.replay_sample(B)
    env._lib.clear()
    for kw in (dict(her=-0.1), dict(her=1.0001), dict(her=None), dict(her='0.5'), dict(her=True), dict(her=float('nan')), dict(strategy='episode'),
               dict(strategy=0), dict(strategy=None), dict(fields=()), dict(fields=('hdr', 'hdr')), dict(fields=('flags',)), dict(seed=-1), dict(seed=2 ** 64),
               dict(seed=1.5), dict(seed=torch.tensor([1, 2])), dict(seed=torch.tensor([1], dtype=torch.int32)), dict(out=dict(r, extra=r['env'])),
               dict(out={f: t for f, t in r.items() if f != 'env'}), dict(out=dict(r, reward=r['reward'].to(torch.int64))),
               dict(out=dict(r, hdr=r['hdr'][:, :8])), dict(fields=('reward',), out=r)):
        raises_before_any_call(env, ValueError, env.replay_sample, B, **kw)
    for b in (-1, 2 ** 27 + 1, 2.0, None, True):
        raises_before_any_call(env, ValueError, env.replay_sample, b)
    raises_before_any_call(env, ValueError, env.replay_sample, B + 1, out=r)


def test_replay_push_takes_actions_as_step_async_does(env):
    if env.host_outputs:
        env.replay_push([0, 5, 7, -1])                             # host actions go through the engine's mapped buffer, as in step_async
        a, dt = the_call(env, 'cw_replay_push', sync=False)
        assert a == env._host_actions.ctypes.data and dt == L.CW_ACT_I32 and env._host_actions.tolist() == [0, 5, -1, -1]
        env.replay_push(np.array([1, 2, 3, 2 ** 40]))
        assert the_call(env, 'cw_replay_push', sync=False)[0] == env._host_actions.ctypes.data and env._host_actions.tolist() == [1, 2, 3, -1]
        raises_before_any_call(env, ValueError, env.replay_push, [0, 1, 2])
        return
    for given, dtype, code in ((torch.tensor([0, 1, 2, 3], dtype=torch.uint8), torch.uint8, L.CW_ACT_U8),
                               (torch.tensor([0, 1, 2, 3], dtype=torch.int64), torch.int64, L.CW_ACT_I64),
                               (torch.tensor([0, 1, 2, 9], dtype=torch.int16), torch.int32, L.CW_ACT_I32), (np.array([4, 5, -1, 6]), torch.int64, L.CW_ACT_I64),
                               ([0, 1, 2, 3], torch.int64, L.CW_ACT_I64)):
        env.replay_push(given)
        a, dt = the_call(env, 'cw_replay_push', sync=False)
        t = at(env, a)                                             # kept alive until the next push
        assert dt == code and t.dtype == dtype and t.is_contiguous() and t.tolist() == torch.as_tensor(np.asarray(given)).tolist()
    same = torch.tensor([0, 1, 2, 3], dtype=torch.int32)
    env.replay_push(same)
    assert the_call(env, 'cw_replay_push', sync=False)[0] == same.data_ptr()       # a tensor of the right kind goes over in place
    raises_before_any_call(env, ValueError, env.replay_push, [0, 1, 2])
    raises_before_any_call(env, ValueError, env.replay_push, torch.zeros(N + 1, dtype=torch.int32))


def test_push_then_step_hand_over_the_same_actions(env):
    if env.host_outputs:
        return
    a = torch.tensor([0, 1, 2, 3], dtype=torch.uint8)
    env._pending, env._actions_keepalive = False, None
    env.replay_push(a)
    env.step_async(a)
    (n1, a1), (n2, a2) = env._lib.calls
    assert (n1, n2) == ('cw_replay_push', 'cw_step') and a1[:2] == a2[:2] == (a.data_ptr(), L.CW_ACT_U8)


def test_replay_clear_and_the_calls_without_a_buffer(env):
    env.replay_clear()
    assert the_call(env, 'cw_replay_clear', sync=False) == ()
    assert env.replay_size() == 0 and env._lib.calls == []         # no buffer: nothing to read, no call
    with pytest.raises(L.CraftingWorldError):
        env.replay_view()
    for bad in (-1, 2 ** 24 + 1, 1.0, None, 2 ** 31 // N + 1):
        raises_before_any_call(env, ValueError, env.replay_reserve, bad)
