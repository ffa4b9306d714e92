"""CPU tier: the host side of plan -- vec_env.plan_args (what cw_plan is handed, validated without a GPU), the ctypes mirror of cw_plan_out against the C
compiler's layout of the header's struct, the ABI entry, and the HIP-free argument rules of cw_plan (cw_host.h: cwh_plan_args)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from hostlib import host_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT32_MAX = 2 ** 31 - 1
N = 7


@pytest.fixture(scope='module')
def lib():
    return host_lib()


def _rec(*lead, pos_dtype=np.int16):
    return np.zeros(lead + (16,), np.uint8), np.zeros(lead + (8,), pos_dtype)


def test_plan_args_accepted_forms():
    from gym_craftingworld_amd.vec_env import EXPAND_FIELDS, PLAN_FIELDS, PLAN_MAX_DEPTH, plan_args
    assert PLAN_FIELDS == ('q', 'length', 'done', 'achieved_mask', 'hdr', 'slot_pos', 'plan', 'best_action', 'best_q') and PLAN_MAX_DEPTH == 8
    assert EXPAND_FIELDS[3:] == PLAN_FIELDS[3:6]
    for depth in range(1, 9):
        assert plan_args(N, depth, None, None, None) == (depth, N)                           # the engine's own states
    assert plan_args(N, np.int64(3), None, None, None) == (3, N)
    assert plan_args(N, 5, *_rec(4), None) == (5, 4)                                         # records: fewer, more, and leading shapes
    assert plan_args(N, 2, *_rec(1000), None) == (2, 1000)
    assert plan_args(N, 2, *_rec(6, N), None) == (2, 6 * N)
    assert plan_args(N, 2, *_rec(3, pos_dtype=np.uint16), None) == (2, 3)
    assert plan_args(N, 4, *_rec(4), [0, N - 1, -1, -7]) == (4, 4)                           # negative: the state takes no part
    assert plan_args(N, 8, *_rec(0), None) == (8, 0)
    assert plan_args(65536, 6, None, None, None) == (6, 65536)                               # the cap: 2^32 plans in one call, at both depths the header names
    assert plan_args(N, 8, *_rec(2048), None) == (8, 2048)
    assert plan_args(N, 6, *_rec(92056), None) == (6, 92056) and plan_args(N, 8, *_rec(2557), None) == (8, 2557)       # ... and the last counts under it
    assert plan_args(N, 4, *_rec(2 ** 20), None) == (4, 2 ** 20)


def test_plan_args_errors():
    from gym_craftingworld_amd.vec_env import plan_args
    hdr, pos = _rec(4)
    for bad in [(0, None, None, None), (9, None, None, None), (-1, None, None, None), (2.0, None, None, None), (True, None, None, None), (None, None, None, None),
                ('3', None, None, None), (0, hdr, pos, None), (9, hdr, pos, None),                                                   # the depth
                (6, *_rec(92057), None), (8, *_rec(2558), None), (8, *_rec(4096), None), (5, *_rec(2 ** 20), None),                  # the cap
                (3, hdr, None, None), (3, None, pos, None), (3, None, None, [0] * N), (3, hdr, _rec(5)[1], None), (3, hdr, pos, [0, 1, 2]),   # expand_args' errors
                (3, hdr, pos, [[0, 1], [2, 3]]), (3, hdr, pos, [0., 1., 2., 3.]), (3, hdr.astype(np.int8), pos, None), (3, hdr, pos.astype(np.int32), None),
                (3, np.zeros((4, 15), np.uint8), pos, None)]:
        with pytest.raises(ValueError):
            plan_args(N, *bad)
    with pytest.raises(ValueError):
        plan_args(92057, 6, None, None, None)
    for bad in ([0, 1, 2, N], [0, 1, 2, INT32_MAX], [N + 31, -1, 0, 0]):         # outside the batch: an IndexError on the host-validated path
        with pytest.raises(IndexError):
            plan_args(N, 3, hdr, pos, bad)


def test_cw_plan_out_mirror_matches_the_header(tmp_path):
    """the ctypes mirror of cw_plan_out has the size and the field offsets the C compiler gives the header's struct (the header stays plain C99)"""
    from gym_craftingworld_amd import _lib
    st = _lib.cw_plan_out
    assert [f for f, _ in st._fields_] == ['q', 'length', 'done', 'achieved', 'hdr', 'slot_pos', 'plan']
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "craftingworld.h"', 'int main(void){',
             'printf("cw_plan_out %zu\\n", sizeof(cw_plan_out));', 'printf("CW_ABI_VERSION %d\\n", CW_ABI_VERSION);']
    for f, _ in st._fields_:
        lines.append('printf("cw_plan_out.%s %%zu\\n", offsetof(cw_plan_out, %s));' % (f, f))
    lines.append('return 0;}')
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-std=c99', '-pedantic', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got['cw_plan_out']) == C.sizeof(st) == 7 * C.sizeof(C.c_void_p)
    for f, _ in st._fields_:
        assert int(got['cw_plan_out.%s' % f]) == getattr(st, f).offset, f
    assert int(got['CW_ABI_VERSION']) == _lib.CW_ABI_VERSION == 5                 # (additive: the number stays)


def test_the_abi_entry():
    from gym_craftingworld_amd import _lib
    res, args = _lib.ABI['cw_plan']
    VP = C.c_void_p
    assert res is C.c_int and args == [VP, VP, VP, VP, C.c_int32, C.c_int32, C.POINTER(_lib.cw_plan_out), VP]
    hdr = open(os.path.join(ROOT, 'include', 'craftingworld.h')).read()
    assert 'int cw_plan(cw_engine *e, const int32_t *env_of, const uint8_t *hdr_in, const uint16_t *slot_pos_in, int32_t n_states, int32_t depth,' in hdr
    assert 'cw_plan_out, cw_plan;' in hdr.split('#define CW_MT_N')[0]             # named in the "added since" list of the version comment


def test_the_argument_rules(lib):
    """cwh_plan_args(num_envs, has env_of, has hdr_in, has slot_pos_in, n_states, depth, output fields) -> which rule refuses the call: cw_expand's rules
    (its own states once, no broadcast), 1 <= depth <= 8 in the place of the steps, and n_states * 6^depth <= 2^32"""
    L, lib = lib
    assert (L.CWH_PLAN_MAX_DEPTH, L.CWH_PLAN_MAX_LEAVES, L.CWH_REC_PLAN_WORK) == (8, 2 ** 32, 7)
    assert 92056 * 6 ** 6 <= 2 ** 32 < 92057 * 6 ** 6 and 2557 * 6 ** 8 <= 2 ** 32 < 2558 * 6 ** 8
    f = lib.cwh_plan_args
    for args in [(N, 0, 0, 0, N, 1, 1), (N, 0, 0, 0, N, 8, 7), (N, 0, 1, 1, 0, 5, 1), (N, 0, 1, 1, 3, 5, 2), (N, 1, 1, 1, 1000, 4, 2), (N, 1, 1, 1, 0, 8, 1),
                 (N, 0, 1, 1, N + 1, 3, 1), (1, 0, 0, 0, 1, 8, 1),
                 (65536, 0, 0, 0, 65536, 6, 1), (N, 0, 1, 1, 65536, 6, 1), (N, 0, 1, 1, 2048, 8, 1), (2048, 0, 0, 0, 2048, 8, 1),        # under the cap
                 (N, 0, 1, 1, 92056, 6, 1), (N, 0, 1, 1, 2557, 8, 1), (N, 0, 1, 1, 2 ** 27, 1, 1),
                 (N, 0, 1, 1, 2 ** 27, 1, 1), (N, 0, 1, 1, 2 ** 20, 4, 1)]:
        assert f(*args) == L.CWH_REC_OK, args
    for args, code in [((N, 0, 0, 0, N, 1, 0), L.CWH_REC_NO_FIELD), ((N, 0, 1, 1, 0, 3, 0), L.CWH_REC_NO_FIELD),
                       ((N, 0, 1, 1, -1, 3, 1), L.CWH_REC_N_STATES), ((N, 0, 1, 1, 2 ** 27 + 1, 1, 1), L.CWH_REC_N_STATES), ((N, 0, 0, 0, -N, 3, 1), L.CWH_REC_N_STATES),
                       ((N, 0, 0, 0, N, 0, 1), L.CWH_REC_N_STEPS), ((N, 0, 0, 0, N, 9, 1), L.CWH_REC_N_STEPS), ((N, 0, 0, 0, N, -1, 1), L.CWH_REC_N_STEPS),
                       ((N, 0, 1, 1, 4, INT32_MAX, 1), L.CWH_REC_N_STEPS), ((N, 0, 1, 1, 4, -2 ** 31, 1), L.CWH_REC_N_STEPS), ((N, 0, 1, 1, 0, 0, 1), L.CWH_REC_N_STEPS),
                       ((N, 0, 1, 1, 92057, 6, 1), L.CWH_REC_PLAN_WORK), ((92057, 0, 0, 0, 92057, 6, 1), L.CWH_REC_PLAN_WORK),       # 92 056 x 6^6 <= 2^32 < 92 057 x 6^6
                       ((N, 0, 1, 1, 4096, 8, 1), L.CWH_REC_PLAN_WORK), ((N, 0, 1, 1, 2558, 8, 1), L.CWH_REC_PLAN_WORK),             # 2 557 x 6^8 <= 2^32 < 2 558 x 6^8
                       ((N, 0, 1, 1, 2 ** 27, 2, 1), L.CWH_REC_PLAN_WORK), ((N, 0, 1, 1, 2 ** 27, 8, 1), L.CWH_REC_PLAN_WORK),
                       ((N, 0, 1, 0, 4, 3, 1), L.CWH_REC_PAIR), ((N, 0, 0, 1, 4, 3, 1), L.CWH_REC_PAIR), ((N, 1, 0, 1, 4, 3, 1), L.CWH_REC_PAIR),
                       ((N, 1, 1, 0, N, 3, 1), L.CWH_REC_PAIR),
                       ((N, 1, 0, 0, N, 3, 1), L.CWH_REC_ENV_OF), ((N, 1, 0, 0, N + 1, 3, 1), L.CWH_REC_ENV_OF),
                       ((N, 0, 0, 0, 0, 3, 1), L.CWH_REC_OWN_STATES), ((N, 0, 0, 0, N - 1, 3, 1), L.CWH_REC_OWN_STATES), ((N, 0, 0, 0, N + 1, 3, 1), L.CWH_REC_OWN_STATES),
                       ((N, 0, 0, 0, 2 * N, 3, 1), L.CWH_REC_OWN_STATES)]:               # (no broadcast: its own states once)
        assert f(*args) == code, (args, code)


def test_the_order_of_the_checks(lib):
    """a call that breaks several rules is refused by the first in the order of cw_host.h: some field, n_states, depth, the cap, the pair, env_of, its own states"""
    L, lib = lib
    f = lib.cwh_plan_args
    order = [L.CWH_REC_NO_FIELD, L.CWH_REC_N_STATES, L.CWH_REC_N_STEPS, L.CWH_REC_PLAN_WORK, L.CWH_REC_PAIR, L.CWH_REC_ENV_OF, L.CWH_REC_OWN_STATES]
    # one argument set per rule that breaks it AND every later one it can be combined with
    assert f(N, 1, 0, 1, -1, 0, 0) == order[0]                    # no field, and n_states, depth, the pair
    assert f(N, 1, 0, 1, -1, 0, 1) == order[1]                    # n_states, and depth, the pair
    assert f(N, 1, 0, 1, 2 ** 27 + 1, 9, 1) == order[1]
    assert f(N, 1, 0, 1, 2 ** 27, 9, 1) == order[2]               # depth, and (were it 8) the cap, and the pair
    assert f(N, 1, 0, 1, 2 ** 27, 8, 1) == order[3]               # the cap, and the pair
    assert f(N, 1, 0, 0, 2 ** 27, 8, 1) == order[3]               # the cap, and env_of without records, and not its own states
    assert f(N, 1, 0, 1, N + 1, 8, 1) == order[4]                 # the pair, and not its own states
    assert f(N, 1, 0, 0, N + 1, 8, 1) == order[5]                 # env_of without records, and not its own states
    assert f(N, 0, 0, 0, N + 1, 8, 1) == order[6]
    assert f(N, 0, 0, 0, N, 8, 1) == L.CWH_REC_OK
    # the codes cw_expand and cw_simulate share keep their numbers
    assert order == [1, 2, 3, 7, 4, 5, 6]
