"""CPU tier: the host side of shoot -- vec_env.shoot_args / shoot_weights (what cw_shoot is handed, validated without a GPU), the ctypes mirror of
cw_shoot_out against the C compiler's layout of the header's struct, the ABI entries, the HIP-free argument rules of cw_shoot and cw_shoot_actions
(cw_host.h: cwh_shoot_args, cwh_shoot_actions_args) and the rule that gives a state its lanes (cwh_shoot_lanes_of)."""
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


def test_shoot_args_accepted_forms():
    from gym_craftingworld_amd.vec_env import SHOOT_FIELDS, SHOOT_MAX_SAMPLES, SHOOT_MAX_WORK, shoot_args, shoot_seed
    assert SHOOT_FIELDS == ('best_ret', 'best_sample', 'best_action', 'length', 'done', 'achieved_mask', 'hdr', 'slot_pos', 'plan', 'ret')
    assert (SHOOT_MAX_SAMPLES, SHOOT_MAX_WORK) == (65536, 2 ** 32)
    assert shoot_args(N, 1, 1, None, None, None) == (1, 1, N)                                 # the engine's own states
    assert shoot_args(N, np.int64(32767), np.int32(2), None, None, None) == (32767, 2, N)
    assert shoot_args(N, 5, 65536, *_rec(4), None) == (5, 65536, 4)
    assert shoot_args(N, 2, 3, *_rec(6, N), None) == (2, 3, 6 * N)
    assert shoot_args(N, 2, 3, *_rec(3, pos_dtype=np.uint16), None) == (2, 3, 3)
    assert shoot_args(N, 4, 4, *_rec(4), [0, N - 1, -1, -7]) == (4, 4, 4)                     # negative: the state takes no part
    assert shoot_args(N, 8, 8, *_rec(0), None) == (8, 8, 0)
    assert shoot_args(65536, 64, 1024, None, None, None) == (64, 1024, 65536)                 # the cap: 2^32 steps in one call
    assert shoot_args(N, 32, 1, *_rec(2 ** 27), None) == (32, 1, 2 ** 27)
    assert [shoot_seed(s) for s in (0, 2 ** 64 - 1, np.int64(5), np.uint64(2 ** 63))] == [0, 2 ** 64 - 1, 5, 2 ** 63]


def test_shoot_args_errors():
    from gym_craftingworld_amd.vec_env import shoot_args, shoot_seed
    hdr, pos = _rec(4)
    for bad in [(0, 1, None, None, None), (32768, 1, None, None, None), (-1, 1, None, None, None), (2.0, 1, None, None, None), (True, 1, None, None, None),
                (None, 1, None, None, None), ('3', 1, None, None, None), (3, 0, None, None, None), (3, 65537, None, None, None), (3, -1, hdr, pos, None),
                (3, 1.0, hdr, pos, None), (3, None, hdr, pos, None), (3, True, hdr, pos, None),
                (64, 1024, *_rec(65537), None), (65, 1024, *_rec(65536), None), (64, 1025, *_rec(65536), None), (33, 1, *_rec(2 ** 27), None),   # the cap
                (3, 2, hdr, None, None), (3, 2, None, pos, None), (3, 2, None, None, [0] * N), (3, 2, hdr, _rec(5)[1], None), (3, 2, hdr, pos, [0, 1, 2]),
                (3, 2, hdr, pos, [0., 1., 2., 3.]), (3, 2, hdr.astype(np.int8), pos, None), (3, 2, np.zeros((4, 15), np.uint8), pos, None)]:
        with pytest.raises(ValueError):
            shoot_args(N, *bad)
    with pytest.raises(IndexError):
        shoot_args(N, 3, 2, hdr, pos, [0, 1, 2, N])
    for bad in (-1, 2 ** 64, 0.0, None, '1', True):
        with pytest.raises(ValueError):
            shoot_seed(bad)


def test_shoot_weights():
    from gym_craftingworld_amd.vec_env import shoot_weights
    w = np.random.RandomState(0).randint(0, 65536, (3, 6, 5))
    for given in (w, w.astype(np.uint16), w.astype(np.int64), w.tolist()):
        got = shoot_weights(given, 3, 5)
        assert got.dtype == np.uint16 and got.flags['C_CONTIGUOUS'] and np.array_equal(got, w)
    got = shoot_weights(w[:, :, 0], 3, 5)                                                     # [T, 6]: every state alike, a copy
    assert got.shape == (3, 6, 5) and got.flags['C_CONTIGUOUS'] and got.flags['OWNDATA'] and (got == w[:, :, :1]).all()
    assert shoot_weights(np.zeros((3, 6, 0), np.uint16), 3, 0).shape == (3, 6, 0)
    for bad in (w.astype(np.float64), w.astype(np.float16), [[0.5] * 6] * 3):
        with pytest.raises(TypeError, match='quantise'):
            shoot_weights(bad, 3, 5)
    for bad in (w[:2], w[:, :5], w[:, :, :4], w - 65536, w + 65535, w.astype(bool), w[:, :, 0].T, np.zeros((3, 6, 5), 'S1')):
        with pytest.raises(ValueError):
            shoot_weights(bad, 3, 5)


def test_cw_shoot_out_mirror_matches_the_header(tmp_path):
    """the ctypes mirror of cw_shoot_out has the size and the field offsets the C compiler gives the header's struct (the header stays plain C99)"""
    from gym_craftingworld_amd import _lib
    st = _lib.cw_shoot_out
    assert [f for f, _ in st._fields_] == ['best_ret', 'best_sample', 'best_action', 'length', 'done', 'achieved', 'hdr', 'slot_pos', 'plan', 'ret']
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "craftingworld.h"', 'int main(void){',
             'printf("cw_shoot_out %zu\\n", sizeof(cw_shoot_out));', 'printf("CW_ABI_VERSION %d\\n", CW_ABI_VERSION);']
    for f, _ in st._fields_:
        lines.append('printf("cw_shoot_out.%s %%zu\\n", offsetof(cw_shoot_out, %s));' % (f, f))
    lines.append('return 0;}')
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-std=c99', '-pedantic', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got['cw_shoot_out']) == C.sizeof(st) == 10 * C.sizeof(C.c_void_p)
    for f, _ in st._fields_:
        assert int(got['cw_shoot_out.%s' % f]) == getattr(st, f).offset, f
    assert int(got['CW_ABI_VERSION']) == _lib.CW_ABI_VERSION == 5                 # (additive: the number stays)


def test_the_abi_entries():
    from gym_craftingworld_amd import _lib
    VP = C.c_void_p
    res, args = _lib.ABI['cw_shoot']
    assert res is C.c_int and args == [VP, VP, VP, VP, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, VP, VP, C.POINTER(_lib.cw_shoot_out), VP]
    res, args = _lib.ABI['cw_shoot_actions']
    assert res is C.c_int and args == [VP, C.c_int32, C.c_int32, C.c_uint64, VP, VP, VP, C.c_int32, VP, VP]
    hdr = open(os.path.join(ROOT, 'include', 'craftingworld.h')).read()
    assert ('int cw_shoot(cw_engine *e, const int32_t *env_of, const uint8_t *hdr_in, const uint16_t *slot_pos_in, int32_t n_states, int32_t n_steps, '
            'int32_t n_samples,') in hdr
    assert 'int cw_shoot_actions(cw_engine *e, int32_t n_states, int32_t n_steps, uint64_t seed, const uint64_t *seed_dev, const uint16_t *weights,' in hdr
    assert 'cw_shoot_out, cw_shoot, cw_shoot_actions;' in hdr.split('#define CW_MT_N')[0]          # named in the "added since" list of the version comment
    for line in ('mix(x):   x ^= x >> 16; x *= 0x7FEB352D; x ^= x >> 15; x *= 0x846CA68B; x ^= x >> 16', 'x = mix((uint32)seed ^ state * 0x9E3779B1)',
                 'x = mix(x ^ ((uint32)(seed >> 32) + sample * 0x85EBCA77))', 'return mix(x ^ step * 0xC2B2AE3D)', 'action(r, w == NULL)   = mulhi32(r, 6)'):
        assert line in hdr, line                                                  # the draw function, verbatim


def test_the_argument_rules_of_cw_shoot(lib):
    """cwh_shoot_args(num_envs, has env_of, has hdr_in, has slot_pos_in, n_states, n_steps, n_samples, output fields) -> which rule refuses the call: cw_plan's
    rules on the records (its own states once), 1 <= n_steps <= 32 767, 1 <= n_samples <= 65 536 and n_states * n_samples * n_steps <= 2^32"""
    L, lib = lib
    assert (L.CWH_SHOOT_MAX_SAMPLES, L.CWH_SHOOT_MAX_WORK, L.CWH_REC_SHOOT_WORK, L.CWH_REC_SHOOT_SAMPLES, L.CWH_SIM_MAX_STEPS) == (65536, 2 ** 32, 8, 9, 32767)
    f = lib.cwh_shoot_args
    for args in [(N, 0, 0, 0, N, 1, 1, 1), (N, 0, 0, 0, N, 32767, 65536 // 8, 10), (N, 0, 1, 1, 0, 5, 5, 1), (N, 0, 1, 1, 3, 5, 65536, 2), (N, 1, 1, 1, 1000, 4, 4, 2),
                 (N, 1, 1, 1, 0, 32767, 65536, 1), (N, 0, 1, 1, N + 1, 3, 3, 1), (1, 0, 0, 0, 1, 32767, 65536, 1),
                 (65536, 0, 0, 0, 65536, 64, 1024, 1), (N, 0, 1, 1, 65536, 64, 1024, 1), (N, 0, 1, 1, 65536, 1024, 64, 1), (N, 0, 1, 1, 2 ** 27, 32, 1, 1),
                 (N, 0, 1, 1, 2 ** 27, 1, 32, 1), (N, 0, 1, 1, 2, 32767, 65536, 1), (N, 0, 1, 1, 4096, 16, 65536, 1)]:                 # the last: exactly 2^32
        assert f(*args) == L.CWH_REC_OK, args
    for args, code in [((N, 0, 0, 0, N, 1, 1, 0), L.CWH_REC_NO_FIELD), ((N, 0, 1, 1, -1, 3, 3, 1), L.CWH_REC_N_STATES), ((N, 0, 1, 1, 2 ** 27 + 1, 1, 1, 1), L.CWH_REC_N_STATES),
                       ((N, 0, 0, 0, N, 0, 1, 1), L.CWH_REC_N_STEPS), ((N, 0, 0, 0, N, 32768, 1, 1), L.CWH_REC_N_STEPS), ((N, 0, 0, 0, N, -1, 1, 1), L.CWH_REC_N_STEPS),
                       ((N, 0, 1, 1, 4, INT32_MAX, 1, 1), L.CWH_REC_N_STEPS), ((N, 0, 1, 1, 4, -2 ** 31, 1, 1), L.CWH_REC_N_STEPS),
                       ((N, 0, 0, 0, N, 3, 0, 1), L.CWH_REC_SHOOT_SAMPLES), ((N, 0, 0, 0, N, 3, 65537, 1), L.CWH_REC_SHOOT_SAMPLES), ((N, 0, 1, 1, 0, 3, -1, 1), L.CWH_REC_SHOOT_SAMPLES),
                       ((N, 0, 1, 1, 4, 3, INT32_MAX, 1), L.CWH_REC_SHOOT_SAMPLES), ((N, 0, 1, 1, 4, 3, -2 ** 31, 1), L.CWH_REC_SHOOT_SAMPLES),
                       ((N, 0, 1, 1, 65537, 64, 1024, 1), L.CWH_REC_SHOOT_WORK), ((N, 0, 1, 1, 65536, 65, 1024, 1), L.CWH_REC_SHOOT_WORK),         # the cap, at its edge
                       ((N, 0, 1, 1, 65536, 64, 1025, 1), L.CWH_REC_SHOOT_WORK), ((65537, 0, 0, 0, 65537, 64, 1024, 1), L.CWH_REC_SHOOT_WORK),
                       ((N, 0, 1, 1, 2 ** 27, 33, 1, 1), L.CWH_REC_SHOOT_WORK), ((N, 0, 1, 1, 3, 32767, 65536, 1), L.CWH_REC_SHOOT_WORK),
                       ((N, 0, 1, 1, 2 ** 27, 32767, 65536, 1), L.CWH_REC_SHOOT_WORK),                                                               # (2^58: no overflow)
                       ((N, 0, 1, 0, 4, 3, 3, 1), L.CWH_REC_PAIR), ((N, 0, 0, 1, 4, 3, 3, 1), L.CWH_REC_PAIR), ((N, 1, 0, 1, 4, 3, 3, 1), L.CWH_REC_PAIR),
                       ((N, 1, 0, 0, N, 3, 3, 1), L.CWH_REC_ENV_OF),
                       ((N, 0, 0, 0, 0, 3, 3, 1), L.CWH_REC_OWN_STATES), ((N, 0, 0, 0, N - 1, 3, 3, 1), L.CWH_REC_OWN_STATES), ((N, 0, 0, 0, 2 * N, 3, 3, 1), L.CWH_REC_OWN_STATES)]:
        assert f(*args) == code, (args, code)


def test_the_order_of_the_checks(lib):
    """a call that breaks several rules is refused by the first in the order of cw_host.h: some field, n_states, n_steps, n_samples, the cap, the pair, env_of,
    its own states"""
    L, lib = lib
    f = lib.cwh_shoot_args
    order = [L.CWH_REC_NO_FIELD, L.CWH_REC_N_STATES, L.CWH_REC_N_STEPS, L.CWH_REC_SHOOT_SAMPLES, L.CWH_REC_SHOOT_WORK, L.CWH_REC_PAIR, L.CWH_REC_ENV_OF,
             L.CWH_REC_OWN_STATES]
    assert f(N, 1, 0, 1, -1, 0, 0, 0) == order[0]
    assert f(N, 1, 0, 1, -1, 0, 0, 1) == order[1]
    assert f(N, 1, 0, 1, 2 ** 27, 0, 0, 1) == order[2]
    assert f(N, 1, 0, 1, 2 ** 27, 64, 0, 1) == order[3]
    assert f(N, 1, 0, 1, 2 ** 27, 64, 1, 1) == order[4]
    assert f(N, 1, 0, 0, 2 ** 27, 64, 1, 1) == order[4]
    assert f(N, 1, 0, 1, N + 1, 64, 1, 1) == order[5]
    assert f(N, 1, 0, 0, N + 1, 64, 1, 1) == order[6]
    assert f(N, 0, 0, 0, N + 1, 64, 1, 1) == order[7]
    assert f(N, 0, 0, 0, N, 64, 1, 1) == L.CWH_REC_OK
    assert order == [1, 2, 3, 9, 8, 4, 5, 6]            # the codes cw_expand, cw_simulate and cw_plan use keep their numbers


def test_the_argument_rules_of_cw_shoot_actions(lib):
    L, lib = lib
    f = lib.cwh_shoot_actions_args
    for args in [(0, 1, 0), (N, 1, 1), (2 ** 27, 32, 1), (1, 32, 2 ** 27), (2 ** 16, 1, 2 ** 16), (65536, 64, 1024), (0, 32767, 2 ** 27), (2 ** 27, 32767, 0)]:
        assert f(*args) == L.CWH_REC_OK, args
    for args, code in [((-1, 1, 1), L.CWH_REC_N_STATES), ((2 ** 27 + 1, 1, 1), L.CWH_REC_N_STATES), ((N, 1, -1), L.CWH_REC_SHOOT_SAMPLES),
                       ((N, 1, 2 ** 27 + 1), L.CWH_REC_SHOOT_SAMPLES), ((N, 0, 1), L.CWH_REC_N_STEPS), ((N, 32768, 1), L.CWH_REC_N_STEPS), ((0, 0, 0), L.CWH_REC_N_STEPS),
                       ((65537, 64, 1024), L.CWH_REC_SHOOT_WORK), ((2 ** 27, 33, 1), L.CWH_REC_SHOOT_WORK), ((2 ** 16, 2, 2 ** 16), L.CWH_REC_SHOOT_WORK),
                       ((2 ** 27, 1, 2 ** 27), L.CWH_REC_SHOOT_WORK), ((2 ** 27, 32767, 2 ** 27), L.CWH_REC_SHOOT_WORK),                      # (2^69 as a product: checked in two steps)
                       ((-1, 0, -1), L.CWH_REC_N_STATES), ((N, 0, -1), L.CWH_REC_SHOOT_SAMPLES)]:
        assert f(*args) == code, (args, code)


def test_the_lanes_of_a_state(lib):
    """cwh_shoot_lanes_of(n_states, n_samples): the smallest power of two G with n_states * G >= 65 536, capped at 64 and at the largest power of two <=
    n_samples -- so one sample is one lane, and a small batch spreads its samples over the wave"""
    _, lib = lib
    f = lib.cwh_shoot_lanes_of
    for m in (1, 65, 600, 1024, 32768, 65536, 2 ** 20):
        prev = None
        for k in range(1, 131):
            g = f(m, k)
            cap = min(64, 1 << (k.bit_length() - 1))
            assert g >= 1 and g & (g - 1) == 0 and g <= min(64, k) and g <= cap, (m, k, g)
            fills = [c for c in (1, 2, 4, 8, 16, 32, 64) if c <= cap and m * c >= 65536]
            assert g == (fills[0] if fills else cap), (m, k, g)          # the smallest that fills the card, else all the rule allows
            assert prev is None or g >= prev                              # more samples never mean fewer lanes
            prev = g
    assert [f(600, k) for k in (1, 2, 3, 5, 8, 16, 33, 64, 100)] == [1, 2, 2, 4, 8, 16, 32, 64, 64]
    assert [f(65, k) for k in (1, 2, 3, 5, 8, 16, 33, 64, 100)] == [1, 2, 2, 4, 8, 16, 32, 64, 64]
    assert [f(1024, k) for k in (1, 33, 64, 130)] == [1, 32, 64, 64] and [f(32768, k) for k in (1, 2, 3, 130)] == [1, 2, 2, 2]
    assert [f(65536, k) for k in (1, 4, 130)] == [1, 1, 1] and f(2 ** 20, 130) == 1 and f(2 ** 27, 65536) == 1 and f(32767, 65536) == 4
