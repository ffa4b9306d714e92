"""CPU tier: the host side of expand -- vec_env.expand_args (what cw_expand is handed, validated without a GPU), the ctypes mirror of cw_expand_out against
the C compiler's layout of the header's struct, and the env-index check cw_expand_kernel shares with the host (cw_host.h: cwh_expand_env_ok)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from hostlib import host_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31
N = 7


@pytest.fixture(scope='module')
def lib():
    return host_lib()[1]


def _rec(*lead, pos_dtype=np.int16):
    return np.zeros(lead + (16,), np.uint8), np.zeros(lead + (8,), pos_dtype)


def test_expand_args_accepted_forms():
    from gym_craftingworld_amd.vec_env import EXPAND_FIELDS, expand_args
    assert EXPAND_FIELDS == ('reward', 'done', 'changed', 'achieved_mask', 'hdr', 'slot_pos')
    assert expand_args(N, None, None, None) == N                                 # the engine's own states
    assert expand_args(N, *_rec(N), None) == N
    assert expand_args(N, *_rec(6, N), None) == 6 * N                            # an earlier result, fed back: depth 2
    assert expand_args(N, *_rec(6, 6, N), None) == 36 * N
    assert expand_args(N, *_rec(3), None) == 3 and expand_args(N, *_rec(1000), None) == 1000      # fewer and more states than envs
    assert expand_args(N, *_rec(0), None) == 0 and expand_args(N, *_rec(0), []) == 0
    assert expand_args(N, *_rec(5, pos_dtype=np.uint16), None) == 5
    assert expand_args(N, *_rec(4), [0, N - 1, -1, -7]) == 4                     # negative: the state takes no part
    assert expand_args(N, *_rec(4), np.array([3, 3, 3, 3], np.int64)) == 4       # repeats: many states of one env
    assert expand_args(N, *_rec(2, 2), [0, 1, 2, 3]) == 4                        # (env_of is flat whatever the records' leading shape)


def test_expand_args_errors():
    from gym_craftingworld_amd.vec_env import expand_args
    hdr, pos = _rec(4)
    for bad in [(hdr, None, None), (None, pos, None),                            # one without the other
                (None, None, [0] * N), (None, None, np.zeros(N, np.int32)),      # env_of without records
                (hdr, _rec(5)[1], None), (_rec(2, 2)[0], pos, None),             # leading shapes that differ
                (hdr, pos, [0, 1, 2]), (hdr, pos, [0, 1, 2, 3, 4]),              # env_of not of length M
                (hdr, pos, [[0, 1], [2, 3]]), (hdr, pos, 2),                     # ... not flat
                (hdr, pos, [0., 1., 2., 3.]), (hdr, pos, ['0', '1', '2', '3']),           # ... not integer
                (hdr.astype(np.int8), pos, None), (hdr, pos.astype(np.int32), None), (hdr, pos.astype(np.float32), None),      # dtypes
                (np.zeros((4, 15), np.uint8), pos, None), (hdr, np.zeros((4, 9), np.int16), None), (np.zeros(16, np.uint8)[:0], pos, None)]:
        with pytest.raises(ValueError):
            expand_args(N, *bad)
    for bad in ([0, 1, 2, N], [0, 1, 2, INT32_MAX], [N + 31, -1, 0, 0]):         # outside the batch: an IndexError on the host-validated path
        with pytest.raises(IndexError):
            expand_args(N, hdr, pos, bad)


def test_cw_expand_out_mirror_matches_the_header(tmp_path):
    """the ctypes mirror of cw_expand_out has the size and the field offsets the C compiler gives the header's struct (the header stays plain C99), and
    CW_NUM_ACTIONS is the header's"""
    from gym_craftingworld_amd import _lib
    st = _lib.cw_expand_out
    assert [f for f, _ in st._fields_] == ['reward', 'done', 'changed', 'achieved', 'hdr', 'slot_pos']
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "craftingworld.h"', 'int main(void){',
             'printf("cw_expand_out %zu\\n", sizeof(cw_expand_out));', 'printf("CW_NUM_ACTIONS %d\\n", CW_NUM_ACTIONS);']
    for f, _ in st._fields_:
        lines.append('printf("cw_expand_out.%s %%zu\\n", offsetof(cw_expand_out, %s));' % (f, f))
    lines.append('return 0;}')
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-std=c99', '-pedantic', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got['cw_expand_out']) == C.sizeof(st) == 6 * C.sizeof(C.c_void_p)
    for f, _ in st._fields_:
        assert int(got['cw_expand_out.%s' % f]) == getattr(st, f).offset, f
    assert int(got['CW_NUM_ACTIONS']) == _lib.CW_NUM_ACTIONS == 6
    assert 'cw_expand' in _lib.ABI and 'cw_export_onehot_states' in _lib.ABI
    assert _lib.ABI['cw_expand'][0] is C.c_int and len(_lib.ABI['cw_expand'][1]) == 7 and len(_lib.ABI['cw_export_onehot_states'][1]) == 6


@pytest.mark.parametrize('num_envs', [1, 70, INT32_MAX])
def test_the_env_check_at_the_extreme_values(lib, num_envs):
    ok = lambda env: lib.cwh_expand_env_in_batch(env, num_envs)      # noqa: E731
    assert ok(0) == 1 and ok(num_envs - 1) == 1
    assert ok(-1) == 0 and ok(num_envs) == 0
    assert ok(INT32_MAX) == 0 and ok(INT32_MIN) == 0 and ok(-7) == 0
    if num_envs < INT32_MAX - 31:
        assert ok(num_envs + 31) == 0
    assert lib.cwh_expand_env_in_batch(0, 0) == 0 and lib.cwh_expand_env_in_batch(INT32_MAX, 0) == 0
