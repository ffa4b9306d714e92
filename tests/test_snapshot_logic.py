"""CPU tier of the device-resident snapshots (cw_snapshot_reserve / _save / _load, CraftingWorldVecEnv.snapshot_*): the comparison the GPU tests rely on
(tests/snapshot_check.py) accepts a correct load and rejects every single-field mutation of it; the host-side row helper (vec_env.snapshot_rows) validates
and packs; the row check shared by host and device holds at the extreme values; the bank's section sizes and offsets; the entry points are declared, bound,
exported and refuse a null engine before they touch HIP.  What the kernels compute is tests/test_snapshot.py's (GPU tier)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from hostlib import host_lib
from snapshot_check import check_load, check_save, sources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31


@pytest.fixture(scope='module')
def lib():
    return host_lib()[1]


# ------------------------------------------------------------------------------------------------------------------------------ the checker
N, S, CAP = 8, 3, 6


def _snap(seed, frames=True):
    """a take()-shaped snapshot of N envs with random content"""
    r = np.random.RandomState(seed)
    u8 = lambda *shape: r.randint(0, 256, shape).astype(np.uint8)      # noqa: E731
    snap = {'state_' + k: u8(N, S, S) for k in ('grid', 'init_grid', 'goal_grid')}
    snap.update({'state_' + k: u8(N, 2) for k in ('agent_rc', 'init_agent_rc', 'goal_agent_rc')})
    snap.update(state_hold=u8(N), state_achieved=r.randint(0, 512, N).astype(np.uint16), state_desired=r.randint(0, 512, N).astype(np.uint16),
                state_step_num=r.randint(0, 17, N).astype(np.int32), state_ep_no=r.randint(0, 9, N).astype(np.int32),
                rng_key=r.randint(0, 2 ** 32, (N, 624), dtype=np.uint64).astype(np.uint32), rng_pos=r.randint(1, 625, N).astype(np.int32),
                hdr=u8(N, 16), slot_pos=r.randint(0, 9, (N, 8)).astype(np.int16), reward=r.randint(-1, 18, N).astype(np.int32), done=u8(N) > 127,
                achieved_mask=r.randint(0, 512, N).astype(np.int16), desired_mask=r.randint(0, 512, N).astype(np.uint16),
                episode_length=r.randint(0, 17, N).astype(np.int32), episode_return=r.randint(-17, 17, N).astype(np.int32),
                counters=r.randint(0, 99, 8).astype(np.int64))
    if frames:
        snap.update({k: u8(N, 4 * S, 4 * S, 3) for k in ('observation', 'desired_goal', 'init_observation')})
    return snap


SAVE_ROWS = np.array([2, -1, 0, 5, 7, -3, 4, 1])         # env 4 names a row outside the bank: rows 0, 1, 2, 4, 5 are saved, 3 never
LOAD_ROWS = np.array([5, 5, -1, 2, 3, 6, 0, -9])         # envs 0, 1 fork env 3; env 3 <- env 0; env 6 <- env 2; env 4: never saved; env 5: outside
GOOD, SRC, BAD = [0, 1, 3, 6], [3, 3, 0, 2], 2


def _by_hand(saved, before, with_stream):
    """the correct result of that load, written out env by env (not the checker's own construction)"""
    after = {k: v.copy() for k, v in before.items()}
    for i, s in zip(GOOD, SRC):
        for k in before:
            if k.startswith('state_') or k in ('slot_pos', 'observation', 'desired_goal', 'init_observation'):
                after[k][i] = saved[k][s]
        menu = before['hdr'][i, 3]
        after['hdr'][i] = saved['hdr'][s]
        after['achieved_mask'][i] = saved['state_achieved'][s]
        after['desired_mask'][i] = saved['state_desired'][s]
        if with_stream:
            after['rng_key'][i], after['rng_pos'][i] = saved['rng_key'][s], saved['rng_pos'][s]
        else:
            after['hdr'][i, 3] = menu
    after['counters'][6] += BAD
    return after


@pytest.mark.parametrize('frames', [True, False])
@pytest.mark.parametrize('with_stream', [True, False])
def test_the_checker_accepts_a_correct_load(with_stream, frames):
    saved, before = _snap(1, frames), _snap(2, frames)
    good, n_bad = check_load(saved, before, _by_hand(saved, before, with_stream), SAVE_ROWS, LOAD_ROWS, with_stream, CAP)
    assert good.tolist() == GOOD and n_bad == BAD
    assert sources(SAVE_ROWS, CAP) == {2: 0, 0: 2, 5: 3, 4: 6, 1: 7}


def _mutations(saved, before, with_stream):
    """(name, mutate(after)) for every single-field mutation the checker must reject"""
    def unchanged_selected(a):
        for k in a:
            if k != 'counters':
                a[k][3] = before[k][3]

    def other_stream(a):                                   # the stream taken where it should be kept, and the reverse
        a['rng_pos'][0] = before['rng_pos'][0] if with_stream else saved['rng_pos'][3]

    def other_key(a):
        a['rng_key'][6] = before['rng_key'][6] if with_stream else saved['rng_key'][2]

    def menu(a):
        a['hdr'][1, 3] = before['hdr'][1, 3] if with_stream else saved['hdr'][3, 3]

    muts = [('a selected row left unchanged', unchanged_selected),
            ('an unselected row changed', lambda a: a['slot_pos'].__setitem__((2, 0), a['slot_pos'][2, 0] + 1)),
            ('a never-saved row loaded', lambda a: a['state_grid'].__setitem__(4, saved['state_grid'][4])),
            ('a row outside the bank loaded', lambda a: a['hdr'].__setitem__(5, saved['hdr'][1])),
            ('the wrong stream position', other_stream), ('the wrong stream key', other_key), ('the menu byte wrong', menu),
            ('reward touched', lambda a: a['reward'].__setitem__(3, a['reward'][3] + 1)),
            ('done touched', lambda a: a['done'].__setitem__(0, not a['done'][0])),
            ('episode_return touched', lambda a: a['episode_return'].__setitem__(6, a['episode_return'][6] - 1)),
            ('counters[6] one short', lambda a: a['counters'].__setitem__(6, a['counters'][6] - 1)),
            ('counters[6] one over', lambda a: a['counters'].__setitem__(6, a['counters'][6] + 1)),
            ('counters[1] touched', lambda a: a['counters'].__setitem__(1, a['counters'][1] + 1)),
            ('the achieved mask stale', lambda a: a['achieved_mask'].__setitem__(0, a['achieved_mask'][0] ^ 1)),
            ('the goal state of the wrong source', lambda a: a['state_goal_grid'].__setitem__(1, saved['state_goal_grid'][0])),
            ('ep_no kept', lambda a: a['state_ep_no'].__setitem__(6, saved['state_ep_no'][2] + 1))]
    if 'observation' in before:
        muts += [('the obs frame not repainted', lambda a: a['observation'].__setitem__((3, 0, 0, 0), a['observation'][3, 0, 0, 0] ^ 1)),
                 ('the init frame not repainted', lambda a: a['init_observation'].__setitem__((0, 1, 1, 1), a['init_observation'][0, 1, 1, 1] ^ 1)),
                 ('the goal frame of an unselected env', lambda a: a['desired_goal'].__setitem__((7, 0, 0, 0), a['desired_goal'][7, 0, 0, 0] ^ 1))]
    return muts


@pytest.mark.parametrize('with_stream', [True, False])
def test_the_checker_rejects_every_single_field_mutation(with_stream):
    saved, before = _snap(3), _snap(4)
    for i in range(N):                                     # (no accidental equality between the two sides of a mutation)
        before['hdr'][i, 3], saved['hdr'][i, 3] = i, 100 + i
    saved['rng_pos'], before['rng_pos'] = np.arange(1, N + 1, dtype=np.int32), np.arange(101, 101 + N, dtype=np.int32)
    right = _by_hand(saved, before, with_stream)
    check_load(saved, before, right, SAVE_ROWS, LOAD_ROWS, with_stream, CAP)
    for name, mutate in _mutations(saved, before, with_stream):
        wrong = {k: v.copy() for k, v in right.items()}
        mutate(wrong)
        assert any(not np.array_equal(wrong[k], right[k]) for k in right), name + ': the mutation changed nothing'
        with pytest.raises(AssertionError):
            check_load(saved, before, wrong, SAVE_ROWS, LOAD_ROWS, with_stream, CAP)
            pytest.fail('not rejected: ' + name)


def test_the_checker_refuses_to_compare_nothing_and_checks_a_save():
    saved, before = _snap(5), _snap(6)
    none = np.array([-1, 7, 3, -2, 6, -1, -1, 99])         # nobody loads a saved row; 7, 3 (never saved), 6 and 99 are bad
    after = {k: v.copy() for k, v in before.items()}
    after['counters'][6] += 4
    with pytest.raises(ValueError):
        check_load(saved, before, after, SAVE_ROWS, none, True, CAP)
    good, n_bad = check_load(saved, before, after, SAVE_ROWS, none, True, CAP, allow_empty=True)
    assert len(good) == 0 and n_bad == 4
    with pytest.raises(ValueError):                        # two envs saved into one row: nothing can be said about it
        check_load(saved, before, after, np.array([1, 1, -1, -1, -1, -1, -1, -1]), none, True, CAP, allow_empty=True)
    with pytest.raises(ValueError):
        check_load(saved, before, after, SAVE_ROWS[:-1], none, True, CAP, allow_empty=True)
    check_save(before, {k: v.copy() for k, v in before.items()})
    for k in ('hdr', 'rng_key', 'counters', 'done'):
        touched = {kk: v.copy() for kk, v in before.items()}
        flat = touched[k].reshape(-1)
        flat[0] = not flat[0] if flat.dtype == np.bool_ else flat[0] ^ 1
        with pytest.raises(AssertionError):
            check_save(before, touched)


# ------------------------------------------------------------------------------------------------------------------------------ snapshot_rows
def test_snapshot_rows_helper():
    from gym_craftingworld_amd.vec_env import snapshot_rows
    got = snapshot_rows(6, 4, [3, -1, 0, -5, 1, 2])
    assert got.dtype == np.int32 and got.flags['C_CONTIGUOUS'] and got.tolist() == [3, -1, 0, -1, 1, 2]          # any negative entry: no part
    assert snapshot_rows(6, 4, [0, 1], envs=[3, 5]).tolist() == [-1, -1, -1, 0, -1, 1]                           # envs paired with rows
    assert snapshot_rows(6, 4, np.array([2, 3], np.int64), envs=np.array([-1, 0])).tolist() == [3, -1, -1, -1, -1, 2]
    assert snapshot_rows(6, 4, [], envs=[]).tolist() == [-1] * 6
    assert snapshot_rows(6, 4, [1, 1, 1, -1, 3, 3], fork=True).tolist() == [1, 1, 1, -1, 3, 3]                   # a load may fork
    assert snapshot_rows(3, 4, [2, 2], envs=[0, 2], fork=True).tolist() == [2, -1, 2]
    assert snapshot_rows(2, INT32_MAX, [INT32_MAX - 1, 0]).tolist() == [INT32_MAX - 1, 0]
    for kw in (dict(rows=[0, 1, 2]),                                   # rows alone: one entry per env
               dict(rows=[0, 1, 2], envs=[0, 1]), dict(rows=[0], envs=[0, 1]),      # lengths that differ
               dict(rows=[0, 1], envs=[2, 2]), dict(rows=[0, 1], envs=[5, -1]),     # an env listed twice (5 and -1 are the same env)
               dict(rows=[0, 4], envs=[0, 1]), dict(rows=[0, 1, 2, 3, 4, 0]), dict(rows=[INT32_MAX] + [-1] * 5),      # a row at or above the capacity
               dict(rows=[1, 1], envs=[0, 1]), dict(rows=[0, 1, 2, 3, 3, -1]),      # a row listed twice for a save
               dict(rows=None), dict(rows=[0.5] * 6), dict(rows=[[0, 1, 2], [3, 0, 1]]), dict(rows=[0], envs=[0.0])):
        with pytest.raises(ValueError):
            snapshot_rows(6, 4, **kw)
    for bad in ([6], [-7]):
        with pytest.raises(IndexError):
            snapshot_rows(6, 4, [0], envs=bad)


# ------------------------------------------------------------------------------------------------------------------------------ the row check
@pytest.mark.parametrize('capacity', [1, 96, INT32_MAX])
def test_the_row_check_at_the_extreme_values(lib, capacity):
    ok = lambda row: lib.cwh_snapshot_row_in_bank(row, capacity)      # noqa: E731
    assert ok(0) == 1 and ok(capacity - 1) == 1
    assert ok(-1) == 0 and ok(capacity) == 0
    assert ok(INT32_MAX) == 0 and ok(INT32_MIN) == 0 and ok(-7) == 0
    assert lib.cwh_snapshot_row_in_bank(0, 0) == 0 and lib.cwh_snapshot_row_in_bank(INT32_MAX, 0) == 0          # no bank: no row


# ------------------------------------------------------------------------------------------------------------------------------ the sections
@pytest.mark.parametrize('la_depth', [0, 4])
@pytest.mark.parametrize('K', [0, 3, 64])
def test_snapshot_section_sizes_and_offsets(lib, K, la_depth):
    L = host_lib()[0]
    n = L.CWH_SNAP_SECTIONS
    for rows in (1, 96, 65536):
        sizes, offs = (C.c_size_t * n)(), (C.c_size_t * n)()
        total, row_bytes = C.c_uint64(), C.c_uint64()
        assert lib.cwh_snapshot_section_bytes(rows, K, la_depth, sizes, offs, C.byref(total), C.byref(row_bytes)) == n
        per_row = [16, 16, 16, 16, 4, 4, 2, 2, 2496, 4, 16 * la_depth, 16 * la_depth, 16 * la_depth, 4 if la_depth else 0, 18 * K, 1]
        assert list(sizes) == [p * rows for p in per_row]
        assert row_bytes.value == sum(per_row) == 2577 + (196 if la_depth else 0) + 18 * K
        end = 0
        for i in range(n):                                 # in order, none overlaps the one before, every start aligned (16-byte records, uint4 stream copies)
            assert offs[i] >= end and offs[i] % L.CWH_SNAP_ALIGN == 0 and offs[i] - end < L.CWH_SNAP_ALIGN
            end = offs[i] + sizes[i]
        assert end <= total.value < end + L.CWH_SNAP_ALIGN
    total, row_bytes = C.c_uint64(7), C.c_uint64(7)
    assert lib.cwh_snapshot_section_bytes(0, K, la_depth, None, None, C.byref(total), C.byref(row_bytes)) == n      # no rows: nothing to allocate
    assert total.value == 0 and row_bytes.value > 0
    assert lib.cwh_snapshot_section_bytes(-5, K, la_depth, None, None, C.byref(total), None) == n and total.value == 0


# ------------------------------------------------------------------------------------------------------------------------------ the C ABI
PROTOTYPES = {
    'cw_snapshot_reserve': r'^int cw_snapshot_reserve\(cw_engine \*e, int32_t rows\);',
    'cw_snapshot_row_bytes': r'^size_t cw_snapshot_row_bytes\(const cw_engine \*e\);',
    'cw_snapshot_save': r'^int cw_snapshot_save\(cw_engine \*e, const int32_t \*rows, cw_stream_t stream\);',
    'cw_snapshot_load': r'^int cw_snapshot_load\(cw_engine \*e, const int32_t \*rows, int32_t with_stream, cw_stream_t stream\);',
}


def test_entry_points_are_declared_bound_and_exported():
    from gym_craftingworld_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, 'include', 'craftingworld.h')).read()
    for name, proto in PROTOTYPES.items():
        assert re.search(proto, hdr, re.M), name
        assert hasattr(lib, name) and name in _lib.ABI
    vp = C.c_void_p
    assert _lib.ABI['cw_snapshot_reserve'] == (C.c_int, [vp, C.c_int32])
    assert _lib.ABI['cw_snapshot_row_bytes'] == (C.c_size_t, [vp])
    assert _lib.ABI['cw_snapshot_save'] == (C.c_int, [vp, vp, vp])
    assert _lib.ABI['cw_snapshot_load'] == (C.c_int, [vp, vp, C.c_int32, vp])
    assert lib.cw_abi_version() == _lib.CW_ABI_VERSION == 5       # (additive: no new ABI number)
    assert 'cw_imagine_masked, cw_sample_state_masked' in hdr and 'cw_snapshot_reserve, cw_snapshot_save' in hdr.split('#define CW_MT_N')[0]


def test_a_null_engine_is_refused_before_any_hip_call():
    from gym_craftingworld_amd import _lib
    lib = _lib.load()
    rows = (C.c_int32 * 4)(0, 1, 2, 3)
    for name, call in (('cw_snapshot_reserve', lambda: lib.cw_snapshot_reserve(None, 4)),
                       ('cw_snapshot_save', lambda: lib.cw_snapshot_save(None, rows, None)),
                       ('cw_snapshot_load', lambda: lib.cw_snapshot_load(None, rows, 1, None))):
        assert call() == _lib.CW_ERR_INVALID, name
        assert name.encode() in lib.cw_last_error(), name
    assert lib.cw_snapshot_row_bytes(None) == 0 and b'cw_snapshot_row_bytes' in lib.cw_last_error()      # (a size, not a status: 0 and the text)
