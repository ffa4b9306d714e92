"""CPU tier: the host side of simulate -- vec_env.simulate_args (what cw_simulate is handed, validated without a GPU), the ctypes mirror of cw_simulate_out
against the C compiler's layout of the header's struct, the ABI entry, and the HIP-free argument rules of cw_simulate and cw_expand (cw_host.h: cwh_records_args,
cwh_ranges_overlap)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from hostlib import host_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT32_MAX = 2 ** 31 - 1
N = 7
U8 = np.dtype(np.uint8)


@pytest.fixture(scope='module')
def lib():
    return host_lib()


def _rec(*lead, pos_dtype=np.int16):
    return np.zeros(lead + (16,), np.uint8), np.zeros(lead + (8,), pos_dtype)


def test_simulate_args_accepted_forms():
    from gym_craftingworld_amd.vec_env import SIMULATE_FIELDS, simulate_args
    assert SIMULATE_FIELDS == ('ret', 'length', 'done', 'achieved_mask', 'hdr', 'slot_pos', 'rewards', 'dones')
    assert simulate_args(N, ((12, N), U8), None, None, None) == (12, N)                      # one plan per env
    assert simulate_args(N, ((12, 3 * N), U8), None, None, None) == (12, 3 * N)              # the broadcast form, flat
    assert simulate_args(N, ((12, 3, N), U8), None, None, None) == (12, 3 * N)               # ... and as [T, K, N]
    assert simulate_args(N, ((1, N), U8), None, None, None) == (1, N)
    assert simulate_args(N, ((32767, 1, N), np.dtype(np.int64)), None, None, None) == (32767, N)
    assert simulate_args(N, ((5, 4), U8), *_rec(4), None) == (5, 4)                          # records: fewer, more, and leading shapes
    assert simulate_args(N, ((5, 1000), np.dtype(np.int32)), *_rec(1000), None) == (5, 1000)
    assert simulate_args(N, ((5, 6, N), U8), *_rec(6, N), None) == (5, 6 * N)
    assert simulate_args(N, ((5, 6 * N), U8), *_rec(6, N), None) == (5, 6 * N)
    assert simulate_args(N, ((5, 3), U8), *_rec(3, pos_dtype=np.uint16), None) == (5, 3)
    assert simulate_args(N, ((9, 4), U8), *_rec(4), [0, N - 1, -1, -7]) == (9, 4)            # negative: the state takes no part
    assert simulate_args(N, ((9, 4), U8), *_rec(4), np.array([3, 3, 3, 3], np.int64)) == (9, 4)
    assert simulate_args(N, ((9, 0), U8), *_rec(0), None) == (9, 0)


def test_simulate_args_errors():
    from gym_craftingworld_amd.vec_env import simulate_args
    hdr, pos = _rec(4)
    for bad in [(((12, N + 1), U8), None, None, None), (((12, 2 * N - 1), U8), None, None, None), (((12, 0), U8), None, None, None),   # M no positive multiple of N
                (((12, 3, N + 1), U8), None, None, None), (((12, 0, N), U8), None, None, None), (((12,), U8), None, None, None),
                (((12, 1, 1, N), U8), None, None, None),
                (((0, N), U8), None, None, None), (((32768, N), U8), None, None, None), (((0, 4), U8), hdr, pos, None),               # T = 0, T = 32 768
                (((32768, 4), U8), hdr, pos, None),
                (((12, N), np.dtype(np.float32)), None, None, None), (((12, N), np.dtype(bool)), None, None, None),                   # a wrong dtype
                (((12, 4), np.dtype(np.float64)), hdr, pos, None),
                (((12, 5), U8), hdr, pos, None), (((12, 3), U8), hdr, pos, None), (((12,), U8), hdr, pos, None),                      # columns != records
                (((12, 4), U8), hdr, None, None), (((12, 4), U8), None, pos, None),                                                   # the expand_args record errors
                (((12, N), U8), None, None, [0] * N), (((12, 4), U8), hdr, _rec(5)[1], None), (((12, 4), U8), hdr, pos, [0, 1, 2]),
                (((12, 4), U8), hdr, pos, [[0, 1], [2, 3]]), (((12, 4), U8), hdr, pos, [0., 1., 2., 3.]),
                (((12, 4), U8), hdr.astype(np.int8), pos, None), (((12, 4), U8), hdr, pos.astype(np.int32), None),
                (((12, 4), U8), np.zeros((4, 15), np.uint8), pos, None)]:
        with pytest.raises(ValueError):
            simulate_args(N, *bad)
    for bad in ([0, 1, 2, N], [0, 1, 2, INT32_MAX], [N + 31, -1, 0, 0]):         # outside the batch: an IndexError on the host-validated path
        with pytest.raises(IndexError):
            simulate_args(N, ((12, 4), U8), hdr, pos, bad)


def test_action_values_on_the_host_path():
    """integers of any width become the uint8 the kernel reads; a value outside 0..255 (an action of 256, a negative one) is refused, not wrapped"""
    from gym_craftingworld_amd.vec_env import simulate_actions
    a = simulate_actions(np.array([[0, 5, 6], [200, 255, 1]], np.int64))
    assert a.dtype == np.uint8 and a.flags.c_contiguous and a.tolist() == [[0, 5, 6], [200, 255, 1]]
    assert simulate_actions(np.arange(12, dtype=np.int16).reshape(3, 4)[:, ::2]).flags.c_contiguous
    for bad in (np.array([[0, 256]]), np.array([[-1, 3]]), np.array([[2 ** 32 + 2, 0]], np.int64), np.array([[1.0, 2.0]]), np.array([[True, False]])):
        with pytest.raises(ValueError):
            simulate_actions(bad)


def test_cw_simulate_out_mirror_matches_the_header(tmp_path):
    """the ctypes mirror of cw_simulate_out has the size and the field offsets the C compiler gives the header's struct (the header stays plain C99)"""
    from gym_craftingworld_amd import _lib
    st = _lib.cw_simulate_out
    assert [f for f, _ in st._fields_] == ['ret', 'length', 'done', 'achieved', 'hdr', 'slot_pos', 'rewards', 'dones']
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "craftingworld.h"', 'int main(void){',
             'printf("cw_simulate_out %zu\\n", sizeof(cw_simulate_out));', 'printf("CW_ABI_VERSION %d\\n", CW_ABI_VERSION);']
    for f, _ in st._fields_:
        lines.append('printf("cw_simulate_out.%s %%zu\\n", offsetof(cw_simulate_out, %s));' % (f, f))
    lines.append('return 0;}')
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-std=c99', '-pedantic', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got['cw_simulate_out']) == C.sizeof(st) == 8 * C.sizeof(C.c_void_p)
    for f, _ in st._fields_:
        assert int(got['cw_simulate_out.%s' % f]) == getattr(st, f).offset, f
    assert int(got['CW_ABI_VERSION']) == _lib.CW_ABI_VERSION == 5                 # (additive: the number stays)


def test_the_abi_entry():
    from gym_craftingworld_amd import _lib
    res, args = _lib.ABI['cw_simulate']
    VP = C.c_void_p
    assert res is C.c_int and args == [VP, VP, VP, VP, C.c_int32, VP, C.c_int32, C.c_int32, C.POINTER(_lib.cw_simulate_out), VP]
    hdr = open(os.path.join(ROOT, 'include', 'craftingworld.h')).read()
    assert 'int cw_simulate(cw_engine *e, const int32_t *env_of, const uint8_t *hdr_in, const uint16_t *slot_pos_in, int32_t n_states,' in hdr
    assert 'cw_simulate_out, cw_simulate)' in hdr.split('#define CW_MT_N')[0]     # named in the "added since" list of the version comment


def test_the_argument_rules(lib):
    """cwh_records_args, the one rule set of a call that reads packed records: (num_envs, has env_of, has hdr_in, has slot_pos_in, n_states, n_steps, output
    fields, max_steps, broadcast) -> which rule refuses the call.  cw_simulate calls it with (32 767, 1), cw_expand -- no steps, its own states once -- with (0, 0)"""
    L, lib = lib
    assert (L.CWH_MAX_STATES, L.CWH_SIM_MAX_STEPS) == (2 ** 27, 32767)

    def f(*args):
        return lib.cwh_records_args(*args, L.CWH_SIM_MAX_STEPS, 1)
    for args in [(N, 0, 0, 0, N, 1, 1), (N, 0, 0, 0, 16 * N, 32767, 8), (N, 0, 1, 1, 0, 5, 1), (N, 0, 1, 1, 3, 5, 2), (N, 1, 1, 1, 1000, 5, 2),
                 (N, 0, 1, 1, 2 ** 27, 1, 1), (1, 0, 0, 0, 2 ** 27, 1, 1), (N, 1, 1, 1, 0, 1, 1)]:
        assert f(*args) == L.CWH_REC_OK, args
    for args, code in [((N, 0, 0, 0, N, 1, 0), L.CWH_REC_NO_FIELD), ((N, 0, 1, 1, 0, 1, 0), L.CWH_REC_NO_FIELD),
                       ((N, 0, 1, 1, -1, 1, 1), L.CWH_REC_N_STATES), ((N, 0, 1, 1, 2 ** 27 + 1, 1, 1), L.CWH_REC_N_STATES),
                       ((N, 0, 1, 1, INT32_MAX, 1, 1), L.CWH_REC_N_STATES), ((N, 0, 0, 0, -N, 1, 1), L.CWH_REC_N_STATES),
                       ((N, 0, 0, 0, N, 0, 1), L.CWH_REC_N_STEPS), ((N, 0, 0, 0, N, -1, 1), L.CWH_REC_N_STEPS), ((N, 0, 0, 0, N, 32768, 1), L.CWH_REC_N_STEPS),
                       ((N, 0, 1, 1, 4, INT32_MAX, 1), L.CWH_REC_N_STEPS), ((N, 0, 1, 1, 4, -2 ** 31, 1), L.CWH_REC_N_STEPS),
                       ((N, 0, 1, 0, 4, 1, 1), L.CWH_REC_PAIR), ((N, 0, 0, 1, 4, 1, 1), L.CWH_REC_PAIR), ((N, 1, 0, 1, 4, 1, 1), L.CWH_REC_PAIR),
                       ((N, 1, 0, 0, N, 1, 1), L.CWH_REC_ENV_OF),
                       ((N, 0, 0, 0, 0, 1, 1), L.CWH_REC_OWN_STATES), ((N, 0, 0, 0, N - 1, 1, 1), L.CWH_REC_OWN_STATES),
                       ((N, 0, 0, 0, N + 1, 1, 1), L.CWH_REC_OWN_STATES), ((N, 0, 0, 0, 2 ** 27, 1, 1), L.CWH_REC_OWN_STATES),
                       ((0, 0, 0, 0, 4, 1, 1), L.CWH_REC_OWN_STATES)]:
        assert f(*args) == code, (args, code)


def test_the_argument_rules_of_expand(lib):
    """the same function as cw_expand calls it: no steps (whatever n_steps holds), and without records n_states is num_envs itself.  Each code is the one
    cw_expand turns into its text (tests/test_expand.py pins the texts on the GPU)"""
    L, lib = lib

    def f(num_envs, env_of, hdr, pos, n_states, fields, n_steps=0):
        return lib.cwh_records_args(num_envs, env_of, hdr, pos, n_states, n_steps, fields, 0, 0)
    for args in [(N, 0, 0, 0, N, 1), (N, 0, 0, 0, N, 6), (1, 0, 0, 0, 1, 1), (2 ** 27, 0, 0, 0, 2 ** 27, 1),          # its own states
                 (N, 0, 1, 1, 0, 1), (N, 0, 1, 1, 3, 2), (N, 0, 1, 1, N - 1, 1), (N, 0, 1, 1, N + 1, 1), (N, 0, 1, 1, 2 ** 27, 1),      # records: any count
                 (N, 1, 1, 1, 1000, 2), (N, 1, 1, 1, 0, 1)]:
        assert f(*args) == L.CWH_REC_OK, args
    for n_steps in (0, -1, 1, 32768, INT32_MAX, -2 ** 31):                           # a call without steps: the value is not looked at
        assert f(N, 0, 0, 0, N, 1, n_steps) == L.CWH_REC_OK, n_steps
    for args, code in [((N, 0, 0, 0, N, 0), L.CWH_REC_NO_FIELD), ((N, 0, 1, 1, 0, 0), L.CWH_REC_NO_FIELD), ((N, 1, 0, 1, -1, 0), L.CWH_REC_NO_FIELD),
                       ((N, 0, 0, 0, -1, 1), L.CWH_REC_N_STATES), ((N, 0, 1, 1, -1, 1), L.CWH_REC_N_STATES), ((N, 0, 0, 0, 2 ** 27 + 1, 1), L.CWH_REC_N_STATES),
                       ((N, 0, 1, 1, 2 ** 27 + 1, 1), L.CWH_REC_N_STATES), ((N, 0, 1, 0, INT32_MAX, 1), L.CWH_REC_N_STATES),
                       ((2 ** 27 + 1, 0, 0, 0, 2 ** 27 + 1, 1), L.CWH_REC_N_STATES),
                       ((N, 0, 1, 0, 4, 1), L.CWH_REC_PAIR), ((N, 0, 0, 1, 4, 1), L.CWH_REC_PAIR), ((N, 1, 0, 1, 4, 1), L.CWH_REC_PAIR), ((N, 1, 1, 0, N, 1), L.CWH_REC_PAIR),
                       ((N, 1, 0, 0, N, 1), L.CWH_REC_ENV_OF), ((N, 1, 0, 0, N + 1, 1), L.CWH_REC_ENV_OF),
                       ((N, 0, 0, 0, 0, 1), L.CWH_REC_OWN_STATES), ((N, 0, 0, 0, N - 1, 1), L.CWH_REC_OWN_STATES), ((N, 0, 0, 0, N + 1, 1), L.CWH_REC_OWN_STATES),
                       ((N, 0, 0, 0, 2 * N, 1), L.CWH_REC_OWN_STATES), ((N, 0, 0, 0, 2 ** 27, 1), L.CWH_REC_OWN_STATES)]:
        assert f(*args) == code, (args, code)


def test_the_overlap_of_two_byte_ranges(lib):
    _, lib = lib
    f = lib.cwh_ranges_overlap
    top = 2 ** 64 - 1
    for a, an, b, bn, want in [(1000, 160, 1000, 160, 1), (1000, 160, 1159, 16, 1), (1000, 160, 1160, 16, 0), (1000, 160, 984, 16, 0), (1000, 160, 985, 16, 1),
                               (1000, 160, 1016, 16, 1), (1016, 16, 1000, 160, 1), (0, 1, 0, 1, 1), (0, 1, 1, 1, 0),
                               (1000, 0, 1000, 160, 0), (1000, 160, 1050, 0, 0), (0, 0, 0, 0, 0),                            # an empty range shares nothing
                               (top - 15, 16, top - 3, 1, 1), (top - 15, 32, 5, 16, 0), (top - 15, 32, top - 1, 1, 1), (top - 15, top, 0, 16, 0),      # no wrap-around
                               (0, top, top - 1, 1, 1), (0, top, top, 1, 0)]:
        assert f(a, an, b, bn) == want, (a, an, b, bn)
        assert f(b, bn, a, an) == want, (b, bn, a, an)
