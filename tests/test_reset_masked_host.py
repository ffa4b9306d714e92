"""CPU tier of the partial reset (cw_reset_masked / CraftingWorldVecEnv.reset_envs): the entry point is declared, bound and exported, refuses null
arguments before it touches HIP, and the host-side mask helper (vec_env.reset_mask) validates and packs what callers hand it.  What the kernel
computes is tests/test_reset_masked.py's (GPU tier)."""
import os
import re

import numpy as np
import pytest

from hostlib import host_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    return host_lib()[1]


def test_entry_point_is_declared_bound_and_exported(lib):
    import ctypes as C
    from gym_craftingworld_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'craftingworld.h')).read()
    assert re.search(r'^int cw_reset_masked\(cw_engine \*e, const uint8_t \*mask, cw_stream_t stream\);', hdr, re.M)
    assert _lib.ABI['cw_reset_masked'] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p])
    assert hasattr(lib, 'cw_reset_masked')
    assert lib.cw_abi_version() == _lib.CW_ABI_VERSION == 5       # (additive: no new ABI number)
    assert 'until cw_reset / cw_reset_masked' in hdr               # (cw_config.auto_reset's comment names both ways out of a finished episode)


def test_null_arguments_are_refused_before_any_hip_call(lib):
    from gym_craftingworld_amd import _lib
    assert lib.cw_reset_masked(None, None, None) == _lib.CW_ERR_INVALID
    assert b'cw_reset_masked' in lib.cw_last_error()


def test_reset_mask_helper():
    from gym_craftingworld_amd.vec_env import reset_mask
    m = reset_mask(6, np.array([True, False, False, True, False, False]))
    assert m.dtype == np.uint8 and m.flags['C_CONTIGUOUS'] and m.tolist() == [1, 0, 0, 1, 0, 0]
    assert reset_mask(4, mask=np.array([0, 7, 0, 255], dtype=np.uint8)).tolist() == [0, 1, 0, 1]         # non-zero = reset
    assert reset_mask(4, [False, True, True, False]).tolist() == [0, 1, 1, 0]
    got = reset_mask(6, indices=[1, 1, -1, 4, -6])                                                      # duplicates, negative ids
    assert got.dtype == np.uint8 and got.tolist() == [1, 1, 0, 0, 1, 1]
    assert reset_mask(6, indices=np.array([2], dtype=np.int32)).tolist() == [0, 0, 1, 0, 0, 0]
    assert reset_mask(6, indices=[]).tolist() == [0] * 6                                                # an empty list is a no-op mask
    for kw in (dict(mask=np.zeros(5, bool)), dict(mask=np.zeros(7, np.uint8)), dict(mask=np.zeros((2, 3), bool)), dict(mask=np.zeros((6, 1), bool)),
               dict(), dict(mask=np.zeros(6, bool), indices=[0]), dict(mask=np.zeros(6, np.float32)), dict(indices=[[0, 1], [2, 3]]),
               dict(indices=[0.5])):
        with pytest.raises(ValueError):
            reset_mask(6, **kw)
    for bad in ([6], [-7], [0, 1, 100]):
        with pytest.raises(IndexError):
            reset_mask(6, indices=bad)
