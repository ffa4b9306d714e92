"""CPU tier: what CraftingWorldVecEnv's methods hand to the library -- entry point and order, scalars, which pointer sits in which slot, what the host
path packs, what comes back, what an empty batch does, what raises before any call, and what is kept alive (tests/recording_engine.py: the env without
an engine, a library that takes notes).  The in-place paths of device tensors are the GPU tier's (tests/test_vec_env_calls_gpu.py)."""
import weakref

import numpy as np
import pytest
import torch

from gym_craftingworld_amd import _lib as L
from recording_engine import kept_tensors, make_env, release

N, S = 4, 5
FRAME = (4 * S, 4 * S, 3)
LEAD, M = (2, 3), 6
EXPAND_SHAPES = {'reward': ((6, M), torch.int32), 'done': ((6, M), torch.bool), 'changed': ((6, M), torch.bool),
                 'achieved_mask': ((6, M), torch.int16), 'hdr': ((6, M, 16), torch.uint8), 'slot_pos': ((6, M, 8), torch.int16)}
STRUCT_OF = {'achieved_mask': 'achieved'}       # the out dict's key -> the member of cw_expand_out / cw_simulate_out


@pytest.fixture(params=[False, True], ids=['device_outputs', 'host_outputs'])
def env(request):
    e = make_env(N, S, host_outputs=request.param)
    yield e
    release(e)


@pytest.fixture
def env2():
    e = make_env(N, S, fixed_init_state=2)
    yield e
    release(e)


def records(lead=LEAD):
    return np.zeros(lead + (16,), np.uint8), np.zeros(lead + (8,), np.int16)


def the_call(env, name, sync=True):
    """the one library call a method made: `name`, followed by exactly one cw_synchronize on a host_outputs engine (sync=False: by none) -> its arguments
    between the engine handle and the stream"""
    want = [name] + (['cw_synchronize'] if sync and env.host_outputs else [])
    assert env._lib.names() == want
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


def raises_before_any_call(env, exc, fn, *a, **kw):
    with pytest.raises(exc):
        fn(*a, **kw)
    assert env._lib.calls == []


# ---------------------------------------------------------------------------------------------------------------- reset_envs
def test_reset_envs(env):
    obs = env.reset_envs(indices=[1])
    (m,) = the_call(env, 'cw_reset_masked')
    packed(env, m, torch.uint8, [0, 1, 0, 0])
    assert set(obs) == {'hdr', 'slot_pos'} and obs['hdr'] is env.hdr and obs['slot_pos'] is env.slot_pos
    env.reset_envs(np.array([True, False, False, True]))
    packed(env, the_call(env, 'cw_reset_masked')[0], torch.uint8, [1, 0, 0, 1])
    env.reset_envs([0, 3, 0, 0])
    packed(env, the_call(env, 'cw_reset_masked')[0], torch.uint8, [0, 1, 0, 0])
    env.reset_envs(torch.tensor([0, 0, 7, 0]))                   # (an int64 tensor: packed on the host)
    packed(env, the_call(env, 'cw_reset_masked')[0], torch.uint8, [0, 0, 1, 0])
    raises_before_any_call(env, ValueError, env.reset_envs)
    raises_before_any_call(env, ValueError, env.reset_envs, [1, 0, 0, 0], indices=[0])
    raises_before_any_call(env, ValueError, env.reset_envs, [1, 0, 0])
    raises_before_any_call(env, IndexError, env.reset_envs, indices=[4])


# ---------------------------------------------------------------------------------------------------------------- imagine_obs / sample_states
def test_imagine_obs(env):
    f = env.imagine_obs()
    m, d, commit, frames, onehot = the_call(env, 'cw_imagine_masked')
    assert (m, d, commit, onehot) == (None, None, 0, None) and frames == f.data_ptr()
    assert f.dtype == torch.uint8 and tuple(f.shape) == (N,) + FRAME
    oh = env.imagine_obs(one_hot=True, commit=True)
    m, d, commit, frames, onehot = the_call(env, 'cw_imagine_masked')
    assert (m, d, commit, frames) == (None, None, 1, None) and onehot == oh.data_ptr()
    assert oh.dtype == torch.uint8 and tuple(oh.shape) == (N, S, S, 12)
    assert env.imagine_obs() is f and env.imagine_obs(one_hot=True) is oh and f is not oh            # scratch: one per kind, reused
    env._lib.clear()
    env.imagine_obs(indices=[-1], desired=[1, 2, 3, 4])
    m, d, commit, frames, onehot = the_call(env, 'cw_imagine_masked')
    packed(env, m, torch.uint8, [0, 0, 0, 1])
    packed(env, d, torch.int16, [1, 2, 3, 4])
    env.imagine_obs([1, 1, 0, 0], desired=np.array([0x8001, 0, 0, 0], np.uint16) & 0x1FF)
    m, d = the_call(env, 'cw_imagine_masked')[:2]
    packed(env, m, torch.uint8, [1, 1, 0, 0])
    packed(env, d, torch.int16, [1, 0, 0, 0])
    rows = np.zeros((N, 9), np.int64)
    rows[2, 8] = 1                                               # task 8 of env 2: bit 8
    env.imagine_obs(desired=rows)
    packed(env, the_call(env, 'cw_imagine_masked')[1], torch.int16, [0, 0, 256, 0])
    out = torch.empty((N,) + FRAME, dtype=torch.uint8)
    assert env.imagine_obs(out=out) is out
    assert the_call(env, 'cw_imagine_masked')[3:] == (out.data_ptr(), None)
    out = torch.empty((N, S, S, 12), dtype=torch.uint8)
    assert env.imagine_obs(out=out, one_hot=True) is out
    assert the_call(env, 'cw_imagine_masked')[3:] == (None, out.data_ptr())
    for bad in (torch.empty((N, S, S, 12), dtype=torch.uint8), torch.empty((N + 1,) + FRAME, dtype=torch.uint8),
                torch.empty((N,) + FRAME, dtype=torch.int8), torch.empty((N, 2) + FRAME, dtype=torch.uint8)[:, 0],
                np.empty((N,) + FRAME, np.uint8)):
        raises_before_any_call(env, ValueError, env.imagine_obs, out=bad)
    raises_before_any_call(env, ValueError, env.imagine_obs, desired=[1, 2, 3, 512])
    raises_before_any_call(env, ValueError, env.imagine_obs, [1, 0, 0, 0], indices=[0])


def test_sample_states(env, env2):
    c = env.sample_states()
    m, pooled, cells = the_call(env, 'cw_sample_state_masked')
    assert (m, pooled) == (None, 0) and cells == c.data_ptr()
    assert c.dtype == torch.uint16 and tuple(c.shape) == (N, 9)
    assert env.sample_states(indices=[2]) is c                   # scratch, reused
    m, pooled, cells = the_call(env, 'cw_sample_state_masked')
    packed(env, m, torch.uint8, [0, 0, 1, 0])
    assert cells == c.data_ptr()
    raises_before_any_call(env, ValueError, env.sample_states, pooled=True)
    env2.sample_states([0, 1, 0, 0], pooled=True)
    m, pooled, _ = the_call(env2, 'cw_sample_state_masked')
    packed(env2, m, torch.uint8, [0, 1, 0, 0])
    assert pooled == 1


# ---------------------------------------------------------------------------------------------------------------- snapshots
def test_snapshots(env):
    assert env.snapshot_save(envs=[1], rows=[2]) is None
    (r,) = the_call(env, 'cw_snapshot_save')
    packed(env, r, torch.int32, [-1, 2, -1, -1])
    env.snapshot_save([3, -7, 0, 1])
    packed(env, the_call(env, 'cw_snapshot_save')[0], torch.int32, [3, -1, 0, 1])
    obs = env.snapshot_load(np.array([5, 5, -1, 5]))             # (a load may fork one row into many envs)
    r, with_stream = the_call(env, 'cw_snapshot_load')
    packed(env, r, torch.int32, [5, 5, -1, 5])
    assert with_stream == 1 and obs['hdr'] is env.hdr
    env.snapshot_load(envs=torch.tensor([-1]), rows=torch.tensor([7]), with_stream=False)
    r, with_stream = the_call(env, 'cw_snapshot_load')
    packed(env, r, torch.int32, [-1, -1, -1, 7])
    assert with_stream == 0
    raises_before_any_call(env, ValueError, env.snapshot_save)
    raises_before_any_call(env, ValueError, env.snapshot_save, [5, 5, -1, -1])          # two envs into one row
    raises_before_any_call(env, ValueError, env.snapshot_save, [8, -1, -1, -1])         # the bank has 8 rows
    raises_before_any_call(env, IndexError, env.snapshot_load, envs=[4], rows=[0])
    env.snapshot_reserve(3)
    assert env._lib.calls == [('cw_synchronize', (None,)), ('cw_snapshot_reserve', (3,))]
    env._lib.clear()
    raises_before_any_call(env, ValueError, env.snapshot_save, [3, -1, -1, -1])         # ... and now 3


# ---------------------------------------------------------------------------------------------------------------- expand
def check_out(out, shapes, struct):
    """the returned dict against the spec, and the struct the library got: a field's member holds its tensor's pointer, every other member is NULL"""
    assert {f: (tuple(t.shape), t.dtype) for f, t in out.items()} == shapes
    assert all(t.is_contiguous() and t.device.type == 'cpu' for t in out.values())
    want = dict.fromkeys(struct)
    want.update({STRUCT_OF.get(f, f): t.data_ptr() for f, t in out.items()})
    assert struct == want


def test_expand(env):
    h, p = records()
    r = env.expand(h, p, [0, 1, 2, 3, -5, 0])
    e, hp, pp, m, struct = the_call(env, 'cw_expand')
    assert m == M and set(struct) == {'reward', 'done', 'changed', 'achieved', 'hdr', 'slot_pos'}
    packed(env, e, torch.int32, [0, 1, 2, 3, -1, 0])
    assert at(env, hp).dtype == torch.uint8 and tuple(at(env, hp).shape) == LEAD + (16,)
    assert at(env, pp).dtype == torch.int16 and tuple(at(env, pp).shape) == LEAD + (8,)
    check_out(r, EXPAND_SHAPES, struct)
    assert env.expand(h, p, out=r) is r                          # an earlier call's dict, written again
    e, hp, pp, m, struct = the_call(env, 'cw_expand')
    assert e is None and m == M
    check_out(r, EXPAND_SHAPES, struct)
    r2 = env.expand(h, p.view(np.uint16), fields=('reward', 'hdr'))
    struct = the_call(env, 'cw_expand')[4]
    check_out(r2, {f: EXPAND_SHAPES[f] for f in ('reward', 'hdr')}, struct)
    assert [k for k, v in struct.items() if v is None] == ['done', 'changed', 'achieved', 'slot_pos']
    own = env.expand()                                           # the engine's own states
    e, hp, pp, m, struct = the_call(env, 'cw_expand')
    assert (e, hp, pp, m) == (None, None, None, N)
    check_out(own, {f: ((6, N) + s[2:], d) for f, (s, d) in EXPAND_SHAPES.items()}, struct)


def test_expand_errors(env):
    h, p = records()
    r = env.expand(h, p)
    env._lib.clear()
    for fields in ((), ('reward', 'nope'), ('reward', 'reward'), ('rewards',)):
        raises_before_any_call(env, ValueError, env.expand, h, p, fields=fields)
    raises_before_any_call(env, ValueError, env.expand, h)                                       # hdr without slot_pos
    raises_before_any_call(env, ValueError, env.expand, None, p)
    raises_before_any_call(env, ValueError, env.expand, env_of=[0, 1, 2, 3])                     # env_of without records
    raises_before_any_call(env, ValueError, env.expand, h, p[:1])
    raises_before_any_call(env, ValueError, env.expand, h.astype(np.int8), p)
    raises_before_any_call(env, ValueError, env.expand, h, p, [0, 1, 2])
    raises_before_any_call(env, IndexError, env.expand, h, p, [0, 1, 2, 3, 4, 0])
    raises_before_any_call(env, ValueError, env.expand, h, p, out={f: r[f] for f in ('reward', 'done')})
    raises_before_any_call(env, ValueError, env.expand, h, p, out=dict(r, extra=r['reward']))
    raises_before_any_call(env, ValueError, env.expand, h, p, fields=('reward',), out={'done': r['done']})
    for f, bad in (('reward', torch.empty((6, M + 1), dtype=torch.int32)), ('reward', torch.empty((6, M), dtype=torch.int64)),
                   ('done', torch.empty((6, M), dtype=torch.uint8)), ('hdr', torch.empty((6, M, 32), dtype=torch.uint8)[:, :, ::2]),
                   ('slot_pos', np.empty((6, M, 8), np.int16))):
        raises_before_any_call(env, ValueError, env.expand, h, p, out=dict(r, **{f: bad}))


# ---------------------------------------------------------------------------------------------------------------- simulate
def sim_shapes(T, m, names):
    spec = {'ret': ((m,), torch.int32), 'length': ((m,), torch.int32), 'done': ((m,), torch.bool), 'achieved_mask': ((m,), torch.int16),
            'hdr': ((m, 16), torch.uint8), 'slot_pos': ((m, 8), torch.int16), 'rewards': ((T, m), torch.int32), 'dones': ((T, m), torch.bool)}
    return {f: spec[f] for f in names}


PER_STATE = ('ret', 'length', 'done', 'achieved_mask', 'hdr', 'slot_pos')


def test_simulate(env):
    a = np.arange(7 * 8, dtype=np.int64).reshape(7, 8) % 9       # the broadcast form: K = 2 plans per env
    r = env.simulate(a)
    e, hp, pp, m, ap, T, stop, struct = the_call(env, 'cw_simulate')
    assert (e, hp, pp, m, T, stop) == (None, None, None, 8, 7, 1)
    packed(env, ap, torch.uint8, a.tolist())                     # int64 actions arrive as uint8
    check_out(r, sim_shapes(7, 8, PER_STATE), struct)
    assert struct['rewards'] is None and struct['dones'] is None
    env.simulate(torch.as_tensor(a).view(7, 2, N), stop_at_done=False)       # [T, K, N]
    m, _, T, stop = the_call(env, 'cw_simulate')[3:7]
    assert (m, T, stop) == (8, 7, 0)
    h, p = records()
    a = [[t % 6] * M for t in range(3)]                          # [3, 6] with records
    r = env.simulate(a, h, p, [0, 1, 2, 3, -5, 0], stop_at_done=False, fields=('ret', 'rewards', 'dones'))
    e, hp, pp, m, ap, T, stop, struct = the_call(env, 'cw_simulate')
    assert (m, T, stop) == (M, 3, 0)
    packed(env, e, torch.int32, [0, 1, 2, 3, -1, 0])
    packed(env, ap, torch.uint8, a)
    assert tuple(at(env, hp).shape) == LEAD + (16,) and tuple(at(env, pp).shape) == LEAD + (8,)
    check_out(r, sim_shapes(3, M, ('ret', 'rewards', 'dones')), struct)
    assert [k for k, v in struct.items() if v is None] == ['length', 'done', 'achieved', 'hdr', 'slot_pos']
    assert env.simulate(np.asarray(a, np.uint8).reshape((3,) + LEAD), h, p, fields=('ret', 'rewards', 'dones'), out=r) is r
    check_out(r, sim_shapes(3, M, ('ret', 'rewards', 'dones')), the_call(env, 'cw_simulate')[7])


def test_simulate_errors(env):
    h, p = records()
    a = np.zeros((3, M), np.uint8)
    r = env.simulate(a, h, p)
    env._lib.clear()
    for fields in ((), ('ret', 'nope'), ('ret', 'ret'), ('reward',)):
        raises_before_any_call(env, ValueError, env.simulate, a, h, p, fields=fields)
    raises_before_any_call(env, ValueError, env.simulate, a, h)
    raises_before_any_call(env, ValueError, env.simulate, a, env_of=[0] * M)
    raises_before_any_call(env, IndexError, env.simulate, a, h, p, [0, 1, 2, 3, 4, 0])
    raises_before_any_call(env, ValueError, env.simulate, a[:, :5], h, p)
    raises_before_any_call(env, ValueError, env.simulate, a)                                      # 6 columns: no multiple of 4 envs
    raises_before_any_call(env, ValueError, env.simulate, a.astype(np.float32), h, p)
    raises_before_any_call(env, ValueError, env.simulate, a.astype(np.int32) + 256, h, p)
    raises_before_any_call(env, ValueError, env.simulate, a[:0], h, p)                            # T = 0
    raises_before_any_call(env, ValueError, env.simulate, a, h, p, out={f: r[f] for f in ('ret', 'done')})
    raises_before_any_call(env, ValueError, env.simulate, a, h, p, out=dict(r, rewards=r['ret']))
    for f, bad in (('ret', torch.empty((M + 1,), dtype=torch.int32)), ('length', torch.empty((M,), dtype=torch.int16)),
                   ('done', torch.empty((M,), dtype=torch.uint8)), ('hdr', torch.empty((M, 32), dtype=torch.uint8)[:, ::2]),
                   ('achieved_mask', [0] * M)):
        raises_before_any_call(env, ValueError, env.simulate, a, h, p, out=dict(r, **{f: bad}))
    raises_before_any_call(env, ValueError, env.simulate, np.zeros((4, M), np.uint8), h, p, fields=('rewards',),
                           out={'rewards': torch.empty((3, M), dtype=torch.int32)})              # T is part of the shape


# ---------------------------------------------------------------------------------------------------------------- one_hot_states / render_records
def test_one_hot_states(env):
    h, p = records()
    o = env.one_hot_states(h, p)
    hp, pp, m, op = the_call(env, 'cw_export_onehot_states')
    assert m == M and op == o.data_ptr() and o.dtype == torch.uint8 and tuple(o.shape) == LEAD + (S, S, 12)
    assert tuple(at(env, hp).shape) == LEAD + (16,) and at(env, pp).dtype == torch.int16
    assert env.one_hot_states(torch.as_tensor(h), torch.as_tensor(p), out=o) is o
    assert the_call(env, 'cw_export_onehot_states')[2:] == (M, o.data_ptr())
    raises_before_any_call(env, ValueError, env.one_hot_states, h, None)
    raises_before_any_call(env, ValueError, env.one_hot_states, None, p)
    raises_before_any_call(env, ValueError, env.one_hot_states, h, p[:1])
    for bad in (torch.empty((M, S, S, 12), dtype=torch.uint8), torch.empty(LEAD + (S, S, 12), dtype=torch.int8),
                torch.empty(LEAD + (S, S, 24), dtype=torch.uint8)[..., ::2], np.empty(LEAD + (S, S, 12), np.uint8)):
        raises_before_any_call(env, ValueError, env.one_hot_states, h, p, out=bad)


def test_render_records(env):
    h, p = records()
    f = env.render_records(h, p)
    hp, pp, mp, m, op = the_call(env, 'cw_render_records')
    assert (mp, m) == (None, M) and op == f.data_ptr() and f.dtype == torch.uint8 and tuple(f.shape) == LEAD + FRAME
    assert tuple(at(env, hp).shape) == LEAD + (16,) and at(env, pp).dtype == torch.int16
    mask = np.arange(M).reshape(LEAD) % 2 == 0
    assert env.render_records(h, p, mask=mask, out=f) is f
    hp, pp, mp, m, op = the_call(env, 'cw_render_records')
    packed(env, mp, torch.uint8, mask.astype(int).tolist())      # a bool mask arrives as bytes
    assert (m, op) == (M, f.data_ptr())
    env.render_records(h, p, mask=torch.as_tensor(mask).to(torch.uint8))
    packed(env, the_call(env, 'cw_render_records')[2], torch.uint8, mask.astype(int).tolist())
    raises_before_any_call(env, ValueError, env.render_records, h, None)
    raises_before_any_call(env, ValueError, env.render_records, None, p)
    raises_before_any_call(env, ValueError, env.render_records, h, p, mask=mask.reshape(-1))
    raises_before_any_call(env, ValueError, env.render_records, h, p, mask=mask.astype(np.int32))
    for bad in (torch.empty((M,) + FRAME, dtype=torch.uint8), torch.empty(LEAD + FRAME, dtype=torch.int16),
                torch.empty(LEAD + FRAME[:2] + (6,), dtype=torch.uint8)[..., ::2], np.empty(LEAD + FRAME, np.uint8)):
        raises_before_any_call(env, ValueError, env.render_records, h, p, out=bad)


@pytest.mark.parametrize('lead', [(0,), (0, 3)])
def test_no_records_no_call(env, lead):
    h, p = records(lead)
    r = env.expand(h, p)
    assert {f: (tuple(t.shape), t.dtype) for f, t in r.items()} == {f: ((6, 0) + s[2:], d) for f, (s, d) in EXPAND_SHAPES.items()}
    assert env.expand(h, p, [], out=r) is r
    s = env.simulate(np.zeros((3,) + lead, np.uint8), h, p, fields=('ret', 'hdr', 'dones'))
    assert {f: (tuple(t.shape), t.dtype) for f, t in s.items()} == sim_shapes(3, 0, ('ret', 'hdr', 'dones'))
    o = env.one_hot_states(h, p)
    assert tuple(o.shape) == lead + (S, S, 12) and o.dtype == torch.uint8
    assert env.one_hot_states(h, p, out=o) is o
    f = env.render_records(h, p, mask=np.zeros(lead, bool))
    assert tuple(f.shape) == lead + FRAME and f.dtype == torch.uint8
    assert env.render_records(h, p, out=f) is f
    assert env._lib.calls == []


# ---------------------------------------------------------------------------------------------------------------- step_many / rollout
def test_step_many(env):
    for dt, code in ((torch.int32, L.CW_ACT_I32), (torch.int64, L.CW_ACT_I64), (torch.uint8, L.CW_ACT_U8)):
        a = torch.zeros((3, N), dtype=dt)
        assert env.step_many(a) is None
        assert the_call(env, 'cw_step_many', sync=False) == (a.data_ptr(), code, 3)
        assert at(env, a.data_ptr()) is a
    for bad in (torch.zeros(N, dtype=torch.int32), torch.zeros((3, 2 * N), dtype=torch.int32)[:, ::2], torch.zeros((3, N + 1), dtype=torch.int32),
                torch.zeros((3, N), dtype=torch.int16), np.zeros((3, N), np.int32), [[0] * N]):
        raises_before_any_call(env, ValueError, env.step_many, bad)


def test_rollout(env):
    a = np.array([[0, 5, 6, -1], [258, 1, 2, 3], [4, 4, 4, 4], [0, 0, 0, 0], [5, 5, 5, 5]])      # int64: outside 0..5 becomes the no-op 255
    rew, don = env.rollout(a)
    ap, T, rp, dp = the_call(env, 'cw_rollout', sync=False)
    packed(env, ap, torch.uint8, [[0, 5, 255, 255], [255, 1, 2, 3], [4, 4, 4, 4], [0, 0, 0, 0], [5, 5, 5, 5]])
    assert T == 5 and (rp, dp) == (rew.data_ptr(), don.data_ptr())
    assert (rew.dtype, don.dtype) == (torch.int32, torch.bool) and tuple(rew.shape) == tuple(don.shape) == (5, N)
    u8 = torch.zeros((2, N), dtype=torch.uint8)
    assert env.rollout(u8, record=False) is None
    assert the_call(env, 'cw_rollout', sync=False) == (u8.data_ptr(), 2, None, None)
    assert at(env, u8.data_ptr()) is u8
    raises_before_any_call(env, ValueError, env.rollout, np.zeros((5, N + 1), np.int64))
    raises_before_any_call(env, ValueError, env.rollout, np.zeros(N, np.int64))


# ---------------------------------------------------------------------------------------------------------------- lifetime
# (method, arguments, entry point, the slots of the pointers that came from the caller's arguments).  Calls in one row of PEERS share a keep-alive
# slot in the env; a call of any other row must leave what the row's last call handed over alone.
CALLS = {
    'reset_envs': (lambda e: e.reset_envs(indices=[1]), 'cw_reset_masked', (0,)),
    'imagine_obs': (lambda e: e.imagine_obs([1, 0, 0, 0], desired=[1, 2, 3, 4]), 'cw_imagine_masked', (0, 1)),
    'sample_states': (lambda e: e.sample_states([1, 0, 0, 0]), 'cw_sample_state_masked', (0,)),
    'snapshot_save': (lambda e: e.snapshot_save(envs=[1], rows=[2]), 'cw_snapshot_save', (0,)),
    'snapshot_load': (lambda e: e.snapshot_load(envs=[1], rows=[2]), 'cw_snapshot_load', (0,)),
    'expand': (lambda e: e.expand(*records(), [0] * M), 'cw_expand', (0, 1, 2)),
    'simulate': (lambda e: e.simulate(np.zeros((3, M), np.int64), *records(), [0] * M), 'cw_simulate', (0, 1, 2, 4)),
    'one_hot_states': (lambda e: e.one_hot_states(*records()), 'cw_export_onehot_states', (0, 1)),
    'render_records': (lambda e: e.render_records(*records(), mask=np.ones(LEAD, bool)), 'cw_render_records', (0, 1, 2)),
    'step_many': (lambda e: e.step_many(torch.zeros((3, N), dtype=torch.int32)), 'cw_step_many', (0,)),
    'rollout': (lambda e: e.rollout(np.zeros((3, N), np.int64)), 'cw_rollout', (0,)),
}
PEERS = [('reset_envs',), ('imagine_obs', 'sample_states'), ('snapshot_save', 'snapshot_load'), ('expand',), ('simulate',), ('one_hot_states',),
         ('render_records',), ('step_many', 'rollout')]


@pytest.mark.parametrize('pick', [0, 1])
def test_what_a_call_handed_over_outlives_calls_of_another_kind(env, pick):
    handed = []                                  # (method, pointer, weak reference to its tensor)
    order = [row[pick % len(row)] for row in PEERS]
    for rounds in range(2):                      # the second round: every slot is overwritten by its own kind, and only by it
        for name in order if rounds == 0 else reversed(order):
            fn, entry, slots = CALLS[name]
            handed = [x for x in handed if x[0] != name]
            fn(env)
            args = the_call(env, entry, sync=entry not in ('cw_step_many', 'cw_rollout'))
            handed += [(name, args[k], weakref.ref(at(env, args[k]))) for k in slots]
            kept = kept_tensors(env)
            for who, ptr, ref in handed:
                assert ref() is not None and kept.get(ptr) is ref(), '%s dropped what %s handed to the library' % (name, who)
