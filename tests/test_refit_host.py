"""CPU tier: the host side of the refit -- vec_env.refit_args (what cw_shoot_refit is handed, validated without a GPU), the ctypes mirror of cw_refit_out
against the C compiler's layout of the header's struct, the ABI entry, and the HIP-free argument rules (cw_host.h: cwh_refit_args): every code, in its
documented order, the caps at their edges, the in-place case accepted and a one-element-shifted overlap refused."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from hostlib import host_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT32_MAX = 2 ** 31 - 1


@pytest.fixture(scope='module')
def lib():
    return host_lib()


def test_refit_args_accepted_forms():
    from gym_craftingworld_amd.vec_env import REFIT_FIELDS, refit_args
    assert REFIT_FIELDS == ('elites', 'weights', 'elite_min')
    i32 = np.int32
    assert refit_args(((8, 5), i32), 3, 6) == (6, 8, 3, 5)
    assert refit_args(((8, 5), i32), 8, 6, 0, 65535) == (6, 8, 8, 5)                         # E = K, smooth 0, the largest gain
    assert refit_args(((1, 5), i32), np.int64(1), np.int32(32767), 65535, 1) == (32767, 1, 1, 5)
    assert refit_args(((65536, 1), i32), 65536, 1) == (1, 65536, 65536, 1)
    assert refit_args(((1024, 65536), i32), 64, 64) == (64, 1024, 64, 65536)                 # the cap: 2^32 draws in one call
    assert refit_args(((4, 0), i32), 2, 3) == (3, 4, 2, 0)
    assert refit_args(((4, 3), i32), 2, 3, env_of=[0, -1, 6], num_envs=7) == (3, 4, 2, 3)
    assert refit_args(((4, 3), i32), 2, 3, env_of=np.array([9, -1, 6]), num_envs=None) == (3, 4, 2, 3)       # (no batch to check against)
    assert refit_args(((4, 0), i32), 2, 3, env_of=[], num_envs=7) == (3, 4, 2, 0)


def test_refit_args_errors():
    from gym_craftingworld_amd.vec_env import refit_args
    i32 = np.int32
    for bad in [(((8, 5), np.int64), 3, 6), (((8, 5), np.float32), 3, 6), (((8,), i32), 3, 6), (((8, 5, 1), i32), 3, 6), (((0, 5), i32), 1, 6),
                (((65537, 1), i32), 1, 6), (((1, 2 ** 27 + 1), i32), 1, 1),
                (((8, 5), i32), 0, 6), (((8, 5), i32), 9, 6), (((8, 5), i32), -1, 6), (((8, 5), i32), 2.0, 6), (((8, 5), i32), None, 6), (((8, 5), i32), True, 6),
                (((8, 5), i32), 3, 0), (((8, 5), i32), 3, 32768), (((8, 5), i32), 3, 6.0), (((8, 5), i32), 3, None),
                (((1024, 65537), i32), 64, 64), (((1025, 65536), i32), 64, 64), (((1024, 65536), i32), 64, 65),                    # the cap, at its edge
                (((8, 5), i32), 3, 6, -1), (((8, 5), i32), 3, 6, 65536), (((8, 5), i32), 3, 6, 1.0), (((8, 5), i32), 3, 6, None),
                (((8, 5), i32), 3, 6, 1, 0), (((8, 5), i32), 3, 6, 1, 65536), (((8, 5), i32), 3, 6, 1, -1), (((8, 5), i32), 3, 6, 1, 2.0),
                (((8, 5), i32), 3, 6, 1, 1, [0, 1, 2, 3]), (((8, 5), i32), 3, 6, 1, 1, [[0, 1, 2, 3, 4]]), (((8, 5), i32), 3, 6, 1, 1, [0., 1., 2., 3., 4.])]:
        with pytest.raises(ValueError):
            refit_args(*bad)
    with pytest.raises(IndexError):
        refit_args(((8, 5), i32), 3, 6, 1, 1, [0, 1, 2, 3, 7], 7)


def test_cw_refit_out_mirror_matches_the_header(tmp_path):
    """the ctypes mirror of cw_refit_out has the size and the field offsets the C compiler gives the header's struct (the header stays plain C99)"""
    from gym_craftingworld_amd import _lib
    st = _lib.cw_refit_out
    assert [f for f, _ in st._fields_] == ['elites', 'weights', 'elite_min']
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "craftingworld.h"', 'int main(void){',
             'printf("cw_refit_out %zu\\n", sizeof(cw_refit_out));', 'printf("CW_ABI_VERSION %d\\n", CW_ABI_VERSION);']
    for f, _ in st._fields_:
        lines.append('printf("cw_refit_out.%s %%zu\\n", offsetof(cw_refit_out, %s));' % (f, f))
    lines.append('return 0;}')
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-std=c99', '-pedantic', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got['cw_refit_out']) == C.sizeof(st) == 3 * C.sizeof(C.c_void_p)
    for f, _ in st._fields_:
        assert int(got['cw_refit_out.%s' % f]) == getattr(st, f).offset, f
    assert int(got['CW_ABI_VERSION']) == _lib.CW_ABI_VERSION == 5                 # (additive: the number stays)


def test_the_abi_entry():
    from gym_craftingworld_amd import _lib
    VP = C.c_void_p
    res, args = _lib.ABI['cw_shoot_refit']
    assert res is C.c_int and args == [VP, VP, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, VP, VP, VP, C.c_uint32, C.c_uint32,
                                       C.POINTER(_lib.cw_refit_out), VP]
    hdr = open(os.path.join(ROOT, 'include', 'craftingworld.h')).read()
    assert ('int cw_shoot_refit(cw_engine *e, const int32_t *env_of, int32_t n_states, int32_t n_steps, int32_t n_samples, int32_t n_elites,\n'
            '                   uint64_t seed, const uint64_t *seed_dev, const uint16_t *weights_in, const int32_t *ret,\n'
            '                   uint32_t smooth, uint32_t gain, const cw_refit_out *out, cw_stream_t stream);') in hdr
    assert 'cw_refit_out, cw_shoot_refit;' in hdr.split('#define CW_MT_N')[0]     # named in the "added since" list of the version comment
    for line in ('min(65535, smooth + gain * c[t][a][j])', '(ret[k][j] DESCENDING, k ASCENDING)', 'ALL T drawn actions of an elite count',
                 'out->weights == weights_in, the same address, is legal', 'It is not counted in counters[7]'):
        assert line in hdr, line                                                  # the semantics, stated where callers read them


# addresses far apart, every buffer of the largest call below fits between two of them
ENV_OF, RET, W_IN, ELITES, W_OUT, EMIN = (0x1000_0000_0000 * i for i in range(1, 7))


def rules(lib, env_of=ENV_OF, m=10, t=3, k=8, e=2, w_in=W_IN, ret=RET, smooth=1, gain=1, elites=ELITES, w_out=W_OUT, emin=EMIN):
    return lib.cwh_refit_args(env_of, m, t, k, e, w_in, ret, smooth, gain, elites, w_out, emin)


def test_the_argument_rules_of_cw_shoot_refit(lib):
    L, lib = lib
    assert [L.CWH_REFIT_OK, L.CWH_REFIT_NULL, L.CWH_REFIT_N_STATES, L.CWH_REFIT_N_STEPS, L.CWH_REFIT_N_SAMPLES, L.CWH_REFIT_N_ELITES, L.CWH_REFIT_WORK,
            L.CWH_REFIT_SMOOTH, L.CWH_REFIT_GAIN, L.CWH_REFIT_ALIGN, L.CWH_REFIT_OVERLAP] == list(range(11))
    ok = L.CWH_REFIT_OK
    for kw in [dict(), dict(env_of=0), dict(w_in=0), dict(w_out=0), dict(emin=0), dict(w_out=0, emin=0, w_in=0, env_of=0), dict(m=0), dict(m=2 ** 27, t=1, k=1, e=1),
               dict(t=32767, k=1, e=1), dict(k=65536, e=65536, m=1), dict(k=65536, e=1, m=1), dict(e=8), dict(smooth=0), dict(smooth=65535), dict(gain=65535),
               dict(m=65536, k=1024, t=64, e=64), dict(m=4096, k=65536, t=16, e=65536), dict(m=0, k=65536, t=32767, e=65536),           # exactly 2^32; no states
               dict(w_in=W_IN + 2, w_out=W_OUT + 2), dict(ret=RET + 4, elites=ELITES + 4, emin=EMIN + 4, env_of=ENV_OF + 4)]:
        assert rules(lib, **kw) == ok, kw
    for kw, code in [(dict(ret=0), L.CWH_REFIT_NULL), (dict(elites=0), L.CWH_REFIT_NULL),
                     (dict(m=-1), L.CWH_REFIT_N_STATES), (dict(m=2 ** 27 + 1, t=1, k=1, e=1), L.CWH_REFIT_N_STATES), (dict(m=-2 ** 31), L.CWH_REFIT_N_STATES),
                     (dict(t=0), L.CWH_REFIT_N_STEPS), (dict(t=32768), L.CWH_REFIT_N_STEPS), (dict(t=-1), L.CWH_REFIT_N_STEPS), (dict(t=INT32_MAX), L.CWH_REFIT_N_STEPS),
                     (dict(k=0, e=0), L.CWH_REFIT_N_SAMPLES), (dict(k=65537), L.CWH_REFIT_N_SAMPLES), (dict(k=-1), L.CWH_REFIT_N_SAMPLES),
                     (dict(e=0), L.CWH_REFIT_N_ELITES), (dict(e=9), L.CWH_REFIT_N_ELITES), (dict(e=-1), L.CWH_REFIT_N_ELITES), (dict(k=1, e=2), L.CWH_REFIT_N_ELITES),
                     (dict(k=65536, e=65537, m=1), L.CWH_REFIT_N_ELITES),                                                                 # E = K + 1
                     (dict(m=65537, k=1024, t=64, e=1), L.CWH_REFIT_WORK), (dict(m=65536, k=1025, t=64, e=1), L.CWH_REFIT_WORK),              # the cap, at its edge
                     (dict(m=65536, k=1024, t=65, e=1), L.CWH_REFIT_WORK), (dict(m=2 ** 27, k=65536, t=32767, e=1), L.CWH_REFIT_WORK),        # (2^58: no overflow)
                     (dict(smooth=65536), L.CWH_REFIT_SMOOTH), (dict(smooth=2 ** 32 - 1), L.CWH_REFIT_SMOOTH),
                     (dict(gain=0), L.CWH_REFIT_GAIN), (dict(gain=65536), L.CWH_REFIT_GAIN), (dict(gain=2 ** 32 - 1), L.CWH_REFIT_GAIN),
                     (dict(env_of=ENV_OF + 2), L.CWH_REFIT_ALIGN), (dict(ret=RET + 1), L.CWH_REFIT_ALIGN), (dict(ret=RET + 2), L.CWH_REFIT_ALIGN),
                     (dict(elites=ELITES + 2), L.CWH_REFIT_ALIGN), (dict(emin=EMIN + 3), L.CWH_REFIT_ALIGN), (dict(w_in=W_IN + 1), L.CWH_REFIT_ALIGN),
                     (dict(w_out=W_OUT + 1), L.CWH_REFIT_ALIGN)]:
        assert rules(lib, **kw) == code, (kw, code)


def test_the_order_of_the_checks(lib):
    """a call that breaks several rules is refused by the first in the order of cw_host.h: null, n_states, n_steps, n_samples, n_elites, the cap, smooth,
    gain, alignment, overlap"""
    L, lib = lib
    worst = dict(ret=0, m=-1, t=0, k=0, e=0, smooth=65536, gain=0, elites=ELITES + 1, w_out=ELITES + 2)
    fixes = [dict(ret=RET), dict(m=2 ** 27), dict(t=32767), dict(k=65536), dict(e=1), dict(m=10, t=3, k=8), dict(smooth=0), dict(gain=1),
             dict(elites=ELITES), dict(w_out=W_OUT)]
    kw = dict(worst)
    for want, fix in zip(range(1, 11), fixes):
        assert rules(lib, **kw) == want, (want, kw)
        kw.update(fix)
    assert rules(lib, **kw) == L.CWH_REFIT_OK


def test_overlaps(lib):
    """no output may share a byte with ret, env_of, another output or weights_in -- but out->weights == weights_in, the same address, is the refit in
    place"""
    L, lib = lib
    ok, bad = L.CWH_REFIT_OK, L.CWH_REFIT_OVERLAP
    m, t, k, e = 10, 3, 8, 2
    sizes = dict(env_of=4 * m, ret=4 * k * m, w_in=12 * t * m, elites=4 * e * m, w_out=12 * t * m, emin=4 * m)
    at = dict(env_of=ENV_OF, ret=RET, w_in=W_IN, elites=ELITES, w_out=W_OUT, emin=EMIN)
    assert rules(lib, w_out=W_IN) == ok                                            # in place
    assert rules(lib, w_out=W_IN + 2) == bad and rules(lib, w_out=W_IN - 2) == bad   # shifted by one element
    assert rules(lib, w_out=W_IN + sizes['w_in'] - 2) == bad and rules(lib, w_out=W_IN + sizes['w_in']) == ok
    assert rules(lib, w_out=W_IN - sizes['w_in'] + 2) == bad and rules(lib, w_out=W_IN - sizes['w_in']) == ok
    assert rules(lib, w_out=W_IN, elites=W_IN + 4) == bad and rules(lib, w_out=W_IN, emin=W_IN + sizes['w_in'] - 4) == bad    # in place excuses the weights only
    for out in ('elites', 'w_out', 'emin'):
        for other in ('env_of', 'ret', 'w_in', 'elites', 'w_out', 'emin'):
            if other == out:
                continue
            step = 4 if out != 'w_out' else 2
            last = at[other] + sizes[other] - step                                 # the last element of the other buffer
            last -= last % 4 if out != 'w_out' else 0
            assert rules(lib, **{out: last}) == bad, (out, other)
            assert rules(lib, **{out: at[other] + sizes[other]}) == ok, (out, other)                 # just behind it
            first = at[other] - sizes[out] + step                                  # the output's last element on the other's first
            assert rules(lib, **{out: first}) == (bad if first % step == 0 else L.CWH_REFIT_ALIGN), (out, other)
            assert rules(lib, **{out: at[other] - sizes[out]}) == ok, (out, other)
    assert rules(lib, m=0, w_out=W_IN + 2, elites=RET, emin=RET) == ok             # no states: no bytes, nothing shared
    assert rules(lib, elites=RET, w_out=0, emin=0) == bad and rules(lib, emin=ELITES, w_out=0) == bad
    assert rules(lib, w_in=0, w_out=W_IN + 2) == ok                                # (no weights_in: nothing there to overlap)
