"""The goal-drawing feature above the kernels, on the CPU: the two entry points in the header / the ctypes table / the library, their argument checks, the
host-side packing of masks and desired vectors, and the N=1 classes' imagine_obs() / sample_state() / generate_fixed_initial_state() replaying the
fixtures captured from the reference (tests/golden/imagine_*.npz) on the fake engine (tests/fake_engine_imagine.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fake_engine_imagine
import imagine_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = M.fixture_names()
CLASSES = {'CraftingWorldEnvRay': 'CraftingWorldEnv', 'CraftingWorldEnvFlat': 'CraftingWorldEnvFlat', 'CraftingWorldEnvOneHot': 'CraftingWorldEnvOneHot',
           'CraftingWorldEnvAltObs': 'CraftingWorldEnvAltObs'}


# ------------------------------------------------------------------------------------------------------------------------------ ABI
def _header():
    return re.sub(r'\s+', ' ', open(os.path.join(ROOT, 'include', 'craftingworld.h')).read())


def test_entry_points_declared_bound_and_exported():
    from gym_craftingworld_amd import _lib as L
    h = _header()
    assert ('int cw_imagine_masked(cw_engine *e, const uint8_t *mask, const uint16_t *desired, int32_t commit, uint8_t *out_frames, uint8_t *out_onehot, '
            'cw_stream_t stream);') in h
    assert 'int cw_sample_state_masked(cw_engine *e, const uint8_t *mask, int32_t pooled, uint16_t *out_cells, cw_stream_t stream);' in h
    assert '#define CW_ABI_VERSION 5' in h and 'cw_imagine_masked, cw_sample_state_masked' in h.split('#define CW_MT_N')[0]
    vp = C.c_void_p
    assert L.ABI['cw_imagine_masked'] == (C.c_int, [vp, vp, vp, C.c_int32, vp, vp, vp])
    assert L.ABI['cw_sample_state_masked'] == (C.c_int, [vp, vp, C.c_int32, vp, vp])
    lib = L.load()
    assert lib.cw_imagine_masked and lib.cw_sample_state_masked and lib.cw_abi_version() == 5
    # each declaration carries the reference lines it replaces
    assert re.search(r'imagine_obs\(\) \(ray\.py:220-299\)', h) and re.search(r'sample_state\(\) \(ray\.py:599-628', h) and 'ray.py:630-644' in h


def test_null_arguments_are_refused_by_name():
    from gym_craftingworld_amd import _lib as L
    lib = L.load()
    buf = (C.c_uint8 * 64)()
    assert lib.cw_imagine_masked(None, None, None, 1, None, None, None) == L.CW_ERR_INVALID
    assert b'cw_imagine_masked' in lib.cw_last_error()
    assert lib.cw_imagine_masked(None, buf, None, 0, buf, None, None) == L.CW_ERR_INVALID
    assert b'cw_imagine_masked' in lib.cw_last_error()
    assert lib.cw_sample_state_masked(None, None, 0, buf, None) == L.CW_ERR_INVALID
    assert b'cw_sample_state_masked' in lib.cw_last_error() and b'engine' in lib.cw_last_error()


# ------------------------------------------------------------------------------------------------------------------------------ packing
def test_desired_bits_packing():
    from gym_craftingworld_amd.vec_env import desired_bits
    rows = np.array([[1, 0, 0, 0, 0, 0, 0, 0, 1], [0] * 9, [1] * 9, [0, 0, 1, 0, 0, 1, 0, 0, 0]])
    assert desired_bits(4, rows, 9).tolist() == [257, 0, 511, 36] and desired_bits(4, rows, 9).dtype == np.uint16
    assert desired_bits(4, rows.astype(bool), 9).tolist() == [257, 0, 511, 36]
    assert desired_bits(3, np.array([1, 511, 0], np.int16), 9).tolist() == [1, 511, 0]
    assert desired_bits(1, np.array([[0, 1, 0, 0, 0, 0, 0, 0, 0]]), 9).tolist() == [2]
    assert desired_bits(1, [0, 1, 0, 0, 0, 0, 0, 0, 0], 9).tolist() == [2]
    for bad in (np.array([512, 0, 0]), np.array([-1, 0, 0]), np.zeros((3, 8), int), np.full((3, 9), 2), np.zeros((2, 9), int), np.zeros(3), [[0.5] * 9] * 3):
        with pytest.raises(ValueError):
            desired_bits(3, bad, 9)
    assert desired_bits(2, np.array([3, 2]), 2).tolist() == [3, 2]           # [N] masks win over an [N, T] reading when N == T


def test_mask_and_indices_follow_reset_envs():
    from gym_craftingworld_amd.vec_env import reset_mask
    assert reset_mask(5, indices=[0, -1]).tolist() == [1, 0, 0, 0, 1]
    with pytest.raises(ValueError):
        reset_mask(5, mask=np.ones(4, bool))
    with pytest.raises(IndexError):
        reset_mask(5, indices=[5])


def test_methods_exist():
    import inspect
    import gym_craftingworld_amd as G
    from gym_craftingworld_amd.adapters import MultiDeviceVecEnv
    from gym_craftingworld_amd.vec_env import CraftingWorldVecEnv
    sig = inspect.signature(CraftingWorldVecEnv.imagine_obs)
    assert list(sig.parameters) == ['self', 'mask', 'indices', 'desired', 'commit', 'out', 'one_hot']
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ('indices', 'desired', 'commit', 'out', 'one_hot'))
    assert list(inspect.signature(CraftingWorldVecEnv.sample_states).parameters) == ['self', 'mask', 'indices', 'pooled']
    for name in ('imagine_obs', 'sample_states'):
        assert callable(getattr(MultiDeviceVecEnv, name))
    for cls in ('CraftingWorldEnv', 'CraftingWorldEnvFlat', 'CraftingWorldEnvOneHot', 'CraftingWorldEnvAltObs'):
        for name in ('imagine_obs', 'sample_state', 'generate_fixed_initial_state'):
            assert callable(getattr(getattr(G.env, cls), name)), (cls, name)
        assert not hasattr(getattr(G.env, cls), 'render_edit') and not hasattr(getattr(G.env, cls), 'eval_task_edit')


# ------------------------------------------------------------------------------------------------------------------------------ the facade
def _make(monkeypatch, name, resident, reference_dtypes):
    import gym_craftingworld_amd.env as E
    fake_engine_imagine.install(monkeypatch, resident=resident)
    meta, kw, d = M.load(name)
    ck = dict(meta['ctor_kwargs'])
    if 'size' in ck:
        ck['size'] = tuple(ck['size'])
    env = getattr(E, CLASSES[meta['env']])(reference_dtypes=reference_dtypes, **ck)
    env.set_rng_state(d['key0'], int(d['pos0']))
    if ck.get('fixed_init_state'):
        env.generate_fixed_states()
    return env, d


def _expected(d, reference_dtypes):
    want = d['rows'].copy()
    want[:, list(M.STATE_COLS)] = np.where(np.isin(d['ops'], (M.I_IMAGINE,))[:, None], 0, want[:, list(M.STATE_COLS)])   # (no probe into the facade's callee)
    if not reference_dtypes:                                   # the frames / states are uint8 unless the caller asked for the reference's dtypes
        img = d['ops'] == M.I_IMAGINE
        want[img, M.COL_DTYPE] = 1 * 4 + 1
    return want


@pytest.mark.parametrize('reference_dtypes', [False, True])
@pytest.mark.parametrize('resident', [True, False])
@pytest.mark.parametrize('name', NAMES)
def test_facade_replays_the_reference(monkeypatch, name, resident, reference_dtypes):
    """returned arrays by CRC, dtype and shape, new objects every call; np_random as the mirror, after a caller's own draw, and as a caller-assigned
    RandomState; an edited desired_goal_vector honoured; env.desired_goal and INIT_OBS_VECTOR unchanged (the flags column)"""
    env, d = _make(monkeypatch, name, resident, reference_dtypes)
    rows, _ = M.run_script(env, d['ops'], d['args'])
    want = _expected(d, reference_dtypes)
    for i in range(len(rows)):
        assert np.array_equal(rows[i], want[i]), 'op %d (%d, arg %d): facade %s, reference %s' % (i, d['ops'][i], d['args'][i], rows[i], want[i])
    env.close()


def test_returns_are_new_arrays_not_views(monkeypatch):
    env, d = _make(monkeypatch, 'imagine_ray5_alias', True, False)
    env.reset()
    a = env.imagine_obs()
    keep = a.copy()
    b = env.imagine_obs()
    assert a is not b and not np.shares_memory(a, b) and np.array_equal(a, keep)
    assert not np.shares_memory(a, env.desired_goal) and a.dtype == np.uint8 and a.shape == env.desired_goal.shape
    s1, p1 = env.sample_state()
    s2, p2 = env.sample_state()
    assert s1 is not s2 and s1.dtype.kind == 'i' and s1.shape == (5, 5, 12) and s1[p1.row, p1.col, 8] == 1 and s1.sum() == 9
    env.close()


def test_generate_fixed_initial_state_without_a_pool(monkeypatch):
    env, d = _make(monkeypatch, 'imagine_ray5_alias', True, False)
    env.reset()
    k, p = env.get_rng_state()
    with pytest.raises(ValueError):
        env.generate_fixed_initial_state()
    k2, p2 = env.get_rng_state()
    assert p2 == p and np.array_equal(k, k2)
    env.close()


def test_pooled_state_is_one_of_the_pool(monkeypatch):
    env, d = _make(monkeypatch, 'imagine_ray6_alias', True, True)
    env.reset()
    pool = env.fixed_state_list
    for _ in range(6):
        state, pos = env.generate_fixed_initial_state()
        assert any(np.array_equal(state, q) for q in pool) and state[pos.row, pos.col, 8] == 1
        assert all(state is not q for q in pool)
    env.close()


def test_imagine_before_reset(monkeypatch):
    env, d = _make(monkeypatch, 'imagine_ray5_alias', True, False)
    with pytest.raises(AttributeError):
        env.imagine_obs()
    env.close()
