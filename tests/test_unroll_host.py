"""CPU tier: the host side of unroll -- vec_env.unroll_args (what cw_unroll is handed, validated without a GPU), the ctypes mirror of cw_unroll_out against
the C compiler's layout of the header's struct, the ABI entry and the version comment, and the HIP-free argument rules of cw_unroll (cw_host.h:
cwh_unroll_args): every code in order, and the cap on one launch's rows on both sides of its edge."""
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


def test_unroll_args_accepted_forms():
    from gym_craftingworld_amd.vec_env import UNROLL_FIELDS, UNROLL_MAX_ROWS, unroll_args
    assert UNROLL_FIELDS == ('hdr', 'slot_pos', 'reward', 'done', 'changed', 'taken', 'length') and UNROLL_MAX_ROWS == 2 ** 27
    assert unroll_args(N, ((12, N), U8), None, None, None) == (12, N)                        # one plan per env
    assert unroll_args(N, ((12, 3 * N), U8), None, None, None) == (12, 3 * N)                # the broadcast form, flat
    assert unroll_args(N, ((12, 3, N), U8), None, None, None) == (12, 3 * N)                 # ... and as [T, K, N]
    assert unroll_args(N, ((1, N), U8), None, None, None) == (1, N)
    assert unroll_args(N, ((32767, 1, N), np.dtype(np.int64)), None, None, None) == (32767, N)
    assert unroll_args(N, ((5, 4), U8), *_rec(4), None) == (5, 4)                            # records: fewer, more, and leading shapes
    assert unroll_args(N, ((5, 1000), np.dtype(np.int32)), *_rec(1000), None) == (5, 1000)
    assert unroll_args(N, ((5, 6, N), U8), *_rec(6, N), None) == (5, 6 * N)
    assert unroll_args(N, ((5, 3), U8), *_rec(3, pos_dtype=np.uint16), None) == (5, 3)
    assert unroll_args(N, ((9, 4), U8), *_rec(4), [0, N - 1, -1, -7]) == (9, 4)              # negative: the state takes no part
    assert unroll_args(N, ((9, 0), U8), *_rec(0), None) == (9, 0)
    assert unroll_args(4096, ((32767, 4096), U8), None, None, None) == (32767, 4096)         # 4 096 * 32 768 = 2**27: the cap itself
    assert unroll_args(1, ((1, 2 ** 26), U8), None, None, None) == (1, 2 ** 26)


def test_unroll_args_errors():
    from gym_craftingworld_amd.vec_env import unroll_args
    hdr, pos = _rec(4)
    for bad in [(((12, N + 1), U8), None, None, None), (((12, 0), U8), None, None, None), (((12, 3, N + 1), U8), None, None, None),     # simulate_args' errors
                (((12,), U8), None, None, None), (((0, N), U8), None, None, None), (((32768, N), U8), None, None, None), (((0, 4), U8), hdr, pos, None),
                (((12, N), np.dtype(np.float32)), None, None, None), (((12, 5), U8), hdr, pos, None), (((12, 4), U8), hdr, None, None),
                (((12, 4), U8), None, pos, None), (((12, N), U8), None, None, [0] * N), (((12, 4), U8), hdr, pos, [0, 1, 2])]:
        with pytest.raises(ValueError):
            unroll_args(N, *bad)
    with pytest.raises(IndexError):
        unroll_args(N, ((12, 4), U8), hdr, pos, [0, 1, 2, N])
    for n, shape in ((4097, (32767, 4097)), (1, (32767, 4097)), (1, (2, 2 ** 26)), (1, (1, 2 ** 27)), (2 ** 13, (32767, 2 ** 13))):       # beyond the cap
        with pytest.raises(ValueError, match='2\\*\\*27'):
            unroll_args(n, (shape, U8), None, None, None)


def test_cw_unroll_out_mirror_matches_the_header(tmp_path):
    """the ctypes mirror of cw_unroll_out has the size and the field offsets the C compiler gives the header's struct: seven pointers"""
    from gym_craftingworld_amd import _lib
    st = _lib.cw_unroll_out
    assert [f for f, _ in st._fields_] == ['hdr', 'slot_pos', 'reward', 'done', 'changed', 'taken', 'length']
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "craftingworld.h"', 'int main(void){',
             'printf("cw_unroll_out %zu\\n", sizeof(cw_unroll_out));', 'printf("CW_ABI_VERSION %d\\n", CW_ABI_VERSION);']
    for f, _ in st._fields_:
        lines.append('printf("cw_unroll_out.%s %%zu\\n", offsetof(cw_unroll_out, %s));' % (f, f))
    lines.append('return 0;}')
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-std=c99', '-pedantic', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got['cw_unroll_out']) == C.sizeof(st) == 7 * C.sizeof(C.c_void_p)
    for f, _ in st._fields_:
        assert int(got['cw_unroll_out.%s' % f]) == getattr(st, f).offset, f
    assert int(got['CW_ABI_VERSION']) == _lib.CW_ABI_VERSION == 5                 # (additive: the number stays)


def test_the_abi_entry_and_the_version_comment():
    from gym_craftingworld_amd import _lib
    res, args = _lib.ABI['cw_unroll']
    VP = C.c_void_p
    assert res is C.c_int and args == [VP, VP, VP, VP, C.c_int32, VP, C.c_int32, C.c_int32, C.POINTER(_lib.cw_unroll_out), VP]
    assert args[:8] == _lib.ABI['cw_simulate'][1][:8]                             # cw_simulate's inputs, argument for argument
    assert _lib.HOST_HELPERS['cwh_unroll_args'] == _lib.HOST_HELPERS['cwh_plan_args']
    hdr = open(os.path.join(ROOT, 'include', 'craftingworld.h')).read()
    assert 'int cw_unroll(cw_engine *e, const int32_t *env_of, const uint8_t *hdr_in, const uint16_t *slot_pos_in, int32_t n_states,' in hdr
    assert 'cw_replay_push, cw_replay_sample; then cw_unroll_out, cw_unroll;' in hdr.split('#define CW_MT_N')[0]
    assert hdr.count('} cw_simulate_out;') == 1 and hdr.count('} cw_unroll_out;') == 1


def test_the_argument_rules(lib):
    """cwh_unroll_args(num_envs, has env_of, has hdr_in, has slot_pos_in, n_states, n_steps, output fields): cw_simulate's rules (cwh_records_args with 32 767
    steps at most, its own states broadcast) with the cap on the rows behind the step check and before the pointer rules"""
    L, lib = lib
    f = lib.cwh_unroll_args
    assert L.CWH_REC_UNROLL_ROWS == 8 and L.CWH_REC_UNROLL_ROWS not in (L.CWH_REC_OK, L.CWH_REC_NO_FIELD, L.CWH_REC_N_STATES, L.CWH_REC_N_STEPS,
                                                                         L.CWH_REC_PAIR, L.CWH_REC_ENV_OF, L.CWH_REC_OWN_STATES)
    for args in [(N, 0, 0, 0, N, 1, 1), (N, 0, 0, 0, 16 * N, 64, 7), (N, 0, 1, 1, 0, 5, 1), (N, 0, 1, 1, 0, 32767, 1), (N, 0, 1, 1, 3, 5, 2),
                 (N, 1, 1, 1, 1000, 5, 2), (N, 1, 1, 1, 0, 1, 1)]:
        assert f(*args) == L.CWH_REC_OK, args
        assert lib.cwh_records_args(*args, L.CWH_SIM_MAX_STEPS, 1) == L.CWH_REC_OK, args
    # every code, in the order the rules are tested: each call breaks the rule of its code and every rule behind it that it can
    for args, code in [((N, 1, 0, 1, -1, 0, 0), L.CWH_REC_NO_FIELD), ((N, 0, 1, 1, 2 ** 27, 32767, 0), L.CWH_REC_NO_FIELD),
                       ((N, 1, 0, 1, -1, 0, 1), L.CWH_REC_N_STATES), ((N, 0, 1, 1, 2 ** 27 + 1, 1, 1), L.CWH_REC_N_STATES),
                       ((N, 0, 1, 1, INT32_MAX, 32767, 1), L.CWH_REC_N_STATES),
                       ((N, 1, 0, 1, 2 ** 27, 0, 1), L.CWH_REC_N_STEPS), ((N, 0, 1, 0, 2 ** 27, 32768, 1), L.CWH_REC_N_STEPS),
                       ((N, 0, 0, 0, N, -1, 1), L.CWH_REC_N_STEPS), ((N, 0, 1, 1, 4, INT32_MAX, 1), L.CWH_REC_N_STEPS),
                       ((N, 1, 0, 1, 2 ** 27, 1, 1), L.CWH_REC_UNROLL_ROWS), ((N, 0, 1, 0, 2 ** 27, 32767, 1), L.CWH_REC_UNROLL_ROWS),
                       ((N, 1, 0, 0, 2 ** 26 + 1, 1, 1), L.CWH_REC_UNROLL_ROWS), ((N, 0, 0, 0, 2 ** 27 - 1, 1, 7), L.CWH_REC_UNROLL_ROWS),
                       ((N, 0, 1, 0, 4, 1, 1), L.CWH_REC_PAIR), ((N, 0, 0, 1, 4, 1, 1), L.CWH_REC_PAIR), ((N, 1, 0, 1, 4, 1, 1), L.CWH_REC_PAIR),
                       ((N, 1, 0, 0, N + 1, 1, 1), L.CWH_REC_ENV_OF),
                       ((N, 0, 0, 0, 0, 1, 1), L.CWH_REC_OWN_STATES), ((N, 0, 0, 0, N - 1, 1, 1), L.CWH_REC_OWN_STATES),
                       ((N, 0, 0, 0, N + 1, 5, 1), L.CWH_REC_OWN_STATES), ((0, 0, 0, 0, 4, 1, 1), L.CWH_REC_OWN_STATES)]:
        assert f(*args) == code, (args, code)


def test_the_cap_on_both_sides_of_its_edge(lib):
    """(n_steps + 1) * n_states <= 2**27: 4 096 states at 32 767 steps are 4 096 * 32 768 = 2**27 records, one state more is refused; 2**26 states take one
    step and not two; the largest batch, 2**27 states, takes none -- with records and in the broadcast form alike"""
    L, lib = lib
    f = lib.cwh_unroll_args
    for records in (1, 0):
        n = 1 if not records else N                                            # (the broadcast form: any count is a multiple of one env)
        assert f(n, 0, records, records, 4096, 32767, 1) == L.CWH_REC_OK
        assert f(n, 0, records, records, 4097, 32767, 1) == L.CWH_REC_UNROLL_ROWS
        assert f(n, 0, records, records, 4096, 32766, 1) == L.CWH_REC_OK
        assert f(n, 0, records, records, 2 ** 26, 1, 1) == L.CWH_REC_OK
        assert f(n, 0, records, records, 2 ** 26, 2, 1) == L.CWH_REC_UNROLL_ROWS
        assert f(n, 0, records, records, 2 ** 26 + 1, 1, 1) == L.CWH_REC_UNROLL_ROWS
        assert f(n, 0, records, records, 2 ** 27, 1, 1) == L.CWH_REC_UNROLL_ROWS
        assert f(n, 0, records, records, 2 ** 12, 2 ** 15 - 1, 1) == L.CWH_REC_OK and f(n, 0, records, records, 2 ** 13, 2 ** 14 - 1, 1) == L.CWH_REC_OK
        assert f(n, 0, records, records, 2 ** 13, 2 ** 14, 1) == L.CWH_REC_UNROLL_ROWS
    from gym_craftingworld_amd.vec_env import unroll_args
    assert unroll_args(1, ((32767, 4096), U8), None, None, None) == (32767, 4096)
    with pytest.raises(ValueError):
        unroll_args(1, ((32767, 4097), U8), None, None, None)
    assert unroll_args(1, ((1, 2 ** 26), U8), None, None, None) == (1, 2 ** 26)
    with pytest.raises(ValueError):
        unroll_args(1, ((2, 2 ** 26), U8), None, None, None)
