"""CPU tests of how the engine reads its CW_TUNE_* variables (csrc/cw_host.cpp: cwh_read_tuning, called once by cw_create's read_tuning):
for each of the 17 variables, unset keeps the default, each documented bound is taken, one step past it keeps the default, and so does text that is not a
whole number -- empty, words, trailing characters, an int that does not fit, nan / inf.  A dict stands in for the process environment."""
import ctypes as C
import math

import pytest

from hostlib import host_lib


# the defaults read_tuning passes in (cw_layout.h CwTuning and cw_engine.cpp; la_period 0 = adaptive, period_ns / rate_tbs -1 = none)
DEFAULTS = dict(render_chunk_rounds=896, step_envs_per_wave=64, gather=1, gather_max_size=7, small_frame_bytes=4096, small_blocks_per_cu=4,
                small_launch_mb=320, reset_blocks_per_cu=4, guard=1, verbose=0, lookahead=1, la_period=0, rollout_segment=-1,
                head_notch=0.4, busy_notch=0.75, period_ns=-1.0, rate_tbs=-1.0)

INT_MAX = 2 ** 31 - 1
# variable -> (field, values taken as themselves, values that keep the default)
INTS = {
    'CW_TUNE_RENDER_CHUNK_ROUNDS': ('render_chunk_rounds', [0, 1, INT_MAX], [-1]),
    'CW_TUNE_STEP_ENVS_PER_WAVE': ('step_envs_per_wave', [8, 16, 32, 64], [0, 7, 9, 12, 24, 63, 65, 128, -8]),
    'CW_TUNE_GATHER_MAX_SIZE': ('gather_max_size', [0, 1, 8, 9], [-1, 10]),
    'CW_TUNE_SMALL_FRAME_BYTES': ('small_frame_bytes', [0, 1, 1048576, INT_MAX], [-1]),
    'CW_TUNE_SMALL_BLOCKS': ('small_blocks_per_cu', [1, 2, 8], [0, 9]),
    'CW_TUNE_SMALL_LAUNCH_MB': ('small_launch_mb', [0, 1, INT_MAX], [-1]),
    'CW_TUNE_RESET_BLOCKS': ('reset_blocks_per_cu', [1, 16], [0, 17]),
    'CW_TUNE_LA_PERIOD': ('la_period', [1, 500, INT_MAX], [0, -1]),
    'CW_TUNE_ROLLOUT_SEGMENT': ('rollout_segment', [-1, 0, 1, 7, INT_MAX], [-2]),
}
REALS = {       # all >= 0
    'CW_TUNE_HEAD_NOTCH': 'head_notch', 'CW_TUNE_BUSY_NOTCH': 'busy_notch', 'CW_TUNE_PERIOD_NS': 'period_ns', 'CW_TUNE_RATE_TBS': 'rate_tbs',
}
FLAGS = {'CW_TUNE_GUARD': 'guard', 'CW_TUNE_LOOKAHEAD': 'lookahead'}       # any int; 0 off, else on
ALL = sorted(list(INTS) + list(REALS) + list(FLAGS) + ['CW_TUNE_GATHER', 'CW_TUNE_VERBOSE'])

MALFORMED_INT = ['', ' ', 'x', 'auto', 'fast', '64k', '8.0', '1e3', '0x10', '8 8', '--8', '+', '2147483648', '-2147483649',
                 '99999999999999999999999', 'nan', 'inf']
MALFORMED_REAL = ['', ' ', 'x', 'fast', '7.7TB', '1.5.2', '0x', 'nan', 'NaN', '-nan', 'inf', 'Infinity', '-inf', '1e999', '-1e999', '1,5']


def read(env):
    """{name: text} -> every field of cwh_tuning after cwh_read_tuning(defaults, env)"""
    L, lib = host_lib()
    bufs = {k.encode(): C.create_string_buffer(v.encode()) for k, v in env.items()}
    asked = []

    def lookup(ctx, name):
        asked.append(name.decode())
        b = bufs.get(name)
        return C.addressof(b) if b is not None else None

    t = L.cwh_tuning(**DEFAULTS)
    lib.cwh_read_tuning(L.cwh_lookup(lookup), None, C.byref(t))
    assert set(asked) == set(ALL), set(asked) ^ set(ALL)            # (every variable is asked for, and nothing else)
    return {f: getattr(t, f) for f in DEFAULTS}


def changed(env):
    got = read(env)
    return {k: v for k, v in got.items() if v != DEFAULTS[k]}


def test_seventeen_variables_unset_keep_every_default():
    assert len(ALL) == 17 == len(DEFAULTS)
    assert read({}) == DEFAULTS
    assert read({'CW_TUNE_SOMETHING_ELSE': '5', 'CW_TUNE_gather': '0'}) == DEFAULTS


@pytest.mark.parametrize('name', sorted(INTS))
def test_integer_variable_bounds(name):
    field, ok, bad = INTS[name]
    for v in ok:
        assert changed({name: str(v)}) == ({field: v} if v != DEFAULTS[field] else {}), (name, v)
    for v in bad:
        assert changed({name: str(v)}) == {}, (name, v)


@pytest.mark.parametrize('name', sorted(INTS) + sorted(FLAGS) + ['CW_TUNE_GATHER'])
def test_integer_variable_malformed_text_keeps_the_default(name):
    for text in MALFORMED_INT:
        assert changed({name: text}) == {}, (name, text)


@pytest.mark.parametrize('name', sorted(INTS))
def test_integer_variable_whitespace_around_the_number(name):
    field, ok, _ = INTS[name]
    v = ok[-1]
    for text in (' %d' % v, '%d ' % v, '\t%d\n' % v, '  +%d  ' % v if v >= 0 else ' %d ' % v):
        assert read({name: text})[field] == v, (name, text)


@pytest.mark.parametrize('name', sorted(REALS))
def test_real_variable_bounds_and_malformed_text(name):
    field = REALS[name]
    for text, v in [('0', 0.0), ('0.0', 0.0), ('-0', 0.0), ('7.7', 7.7), (' 6.25 ', 6.25), ('1e3', 1000.0), ('5', 5.0), ('1e300', 1e300)]:
        assert read({name: text})[field] == v, (name, text)
    for text in ['-1', '-0.001', '-1e-300'] + MALFORMED_REAL:
        assert changed({name: text}) == {}, (name, text)


def test_the_malformed_values_that_used_to_read_as_zero():
    """atoi / atof read any text that is not a number as 0, a valid value of these five: an unclocked sweep, one launch for the whole batch, no
    look-ahead, no small-frame path"""
    for name, text in [('CW_TUNE_PERIOD_NS', 'fast'), ('CW_TUNE_RATE_TBS', 'x'), ('CW_TUNE_RENDER_CHUNK_ROUNDS', 'auto'), ('CW_TUNE_LOOKAHEAD', ''),
                       ('CW_TUNE_SMALL_FRAME_BYTES', 'x'), ('CW_TUNE_GUARD', 'off'), ('CW_TUNE_ROLLOUT_SEGMENT', 'none'), ('CW_TUNE_GATHER', 'no')]:
        assert changed({name: text}) == {}, (name, text)
    assert changed({'CW_TUNE_SMALL_LAUNCH_MB': '320MB', 'CW_TUNE_LA_PERIOD': '64k', 'CW_TUNE_RESET_BLOCKS': '4294967297'}) == {}


def test_flags_and_gather_take_any_int():
    for name, field in FLAGS.items():
        assert read({name: '0'})[field] == 0 and read({name: ' 0 '})[field] == 0 and read({name: '-0'})[field] == 0
        for text in ('1', '2', '-1', str(INT_MAX), str(-INT_MAX - 1)):
            assert read({name: text})[field] == 1, (name, text)
    for text, v in (('0', 0), ('1', 1), ('-3', -3), (str(INT_MAX), INT_MAX), (str(-INT_MAX - 1), -INT_MAX - 1)):
        assert read({'CW_TUNE_GATHER': text})['gather'] == v


def test_verbose_is_on_when_set_at_all():
    """CW_TUNE_VERBOSE is a presence flag (pinned): set to anything, '0' and '' included, it is on"""
    for text in ('1', '0', '', 'no', 'x'):
        assert changed({'CW_TUNE_VERBOSE': text}) == {'verbose': 1}, text


def test_special_sets():
    """the variables whose valid values are not a plain half-line"""
    assert [v for v in range(-2, 130) if read({'CW_TUNE_STEP_ENVS_PER_WAVE': str(v)})['step_envs_per_wave'] == v] == [8, 16, 32, 64]
    assert [v for v in range(-2, 12) if read({'CW_TUNE_GATHER_MAX_SIZE': str(v)})['gather_max_size'] == v] == list(range(10))
    ok = [v for v in range(-2, 20) if read({'CW_TUNE_RESET_BLOCKS': str(v)})['reset_blocks_per_cu'] == v]
    assert ok == list(range(1, 17))
    assert [v for v in range(-2, 12) if read({'CW_TUNE_SMALL_BLOCKS': str(v)})['small_blocks_per_cu'] == v] == list(range(1, 9))
    assert read({'CW_TUNE_LA_PERIOD': '0'})['la_period'] == 0                    # (0: adaptive, the engine's default -- also the value 0 itself)
    assert [v for v in range(-4, 3) if read({'CW_TUNE_ROLLOUT_SEGMENT': str(v)})['rollout_segment'] == v] == [-1, 0, 1, 2]
    # the default kept by a rejected value is the one passed in, not a constant
    L, lib = host_lib()
    t = L.cwh_tuning(**dict(DEFAULTS, step_envs_per_wave=16, rollout_segment=5, period_ns=3.5))
    lib.cwh_read_tuning(L.cwh_lookup(lambda ctx, name: None), None, C.byref(t))
    assert (t.step_envs_per_wave, t.rollout_segment, t.period_ns) == (16, 5, 3.5)


def test_many_variables_at_once():
    env = {'CW_TUNE_STEP_ENVS_PER_WAVE': '16', 'CW_TUNE_GATHER_MAX_SIZE': '9', 'CW_TUNE_RESET_BLOCKS': '16', 'CW_TUNE_LA_PERIOD': '1',
           'CW_TUNE_ROLLOUT_SEGMENT': '0', 'CW_TUNE_PERIOD_NS': '0', 'CW_TUNE_RATE_TBS': 'fast', 'CW_TUNE_LOOKAHEAD': '0',
           'CW_TUNE_SMALL_FRAME_BYTES': '1048576', 'CW_TUNE_SMALL_BLOCKS': '8', 'CW_TUNE_HEAD_NOTCH': '0.25'}
    assert changed(env) == dict(step_envs_per_wave=16, gather_max_size=9, reset_blocks_per_cu=16, la_period=1, rollout_segment=0, period_ns=0.0,
                                lookahead=0, small_frame_bytes=1048576, small_blocks_per_cu=8, head_notch=0.25)
    assert math.isclose(read(env)['busy_notch'], 0.75)
