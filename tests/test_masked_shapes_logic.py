"""CPU tier: the comparison of tests/masked_check.py itself (what tests/test_masked_shapes.py relies on), on snapshots built without a GPU -- the
"before" side from the CPU oracle, the "after" side by this file's own use of the model: a faithful after-snapshot passes, and every way a masked
kernel can be wrong that the GPU tests are there to catch -- one element of any compared quantity in a selected row, one element of an unselected
row, a kernel that stops before the last partial chunk, two envs' results swapped within a chunk -- fails, naming the quantity and the env."""
import ctypes as C

import numpy as np
import pytest

import imagine_model as M
from hostlib import host_lib
from masked_check import check_masked_call, masked_launch, untouched
from oracle_replay import oracle_arrays

N, S, EPB = 37, 5, 8


def _before(pixels):
    from oracle import OracleBatch
    ora = OracleBatch(N, rng_states=[tuple(np.random.RandomState(700 + i).get_state()[1:3]) for i in range(N)], size=(S, S), max_steps=9)
    ora.reset()
    acts = np.random.RandomState(1).randint(0, 4, (12, N))
    for t in range(12):
        ora.step(acts[t])
    arr = oracle_arrays(ora.envs, ['rng_key'] + (['observation', 'desired_goal', 'init_observation'] if pixels else []))
    snap = {'state_' + k: np.ascontiguousarray(v).astype(np.int32 if k in ('step_num', 'ep_no') else np.uint16 if k in ('achieved', 'desired') else np.uint8)
            for k, v in arr.items() if not k.startswith('rng_') and k not in ('observation', 'desired_goal', 'init_observation')}
    snap['rng_key'], snap['rng_pos'] = arr['rng_key'], arr['rng_pos']
    hdr = np.random.RandomState(2).randint(0, 256, (N, 16)).astype(np.uint8)
    hdr[:, 6], hdr[:, 7] = snap['state_desired'] & 0xFF, snap['state_desired'] >> 8
    snap.update(hdr=hdr, slot_pos=np.arange(N * 4, dtype=np.uint32).reshape(N, 4), reward=np.full(N, -1, np.int32), done=np.zeros(N, np.uint8),
                achieved_mask=snap['state_achieved'].astype(np.int16), desired_mask=snap['state_desired'].copy(), episode_length=np.arange(N, dtype=np.int32),
                episode_return=-np.arange(N, dtype=np.int32), counters=np.arange(8, dtype=np.uint64))
    for k in ('observation', 'desired_goal', 'init_observation'):
        if pixels:
            snap[k] = arr[k]
    on_start = (snap['state_agent_rc'] == snap['state_init_agent_rc']).all(axis=1)
    assert on_start.any() and (~on_start).any()
    return snap


def _imagine_after(before, sel, desired, commit, upto=N):
    """what a correct cw_imagine_masked leaves and returns for the selected envs below `upto` -> (after, frames, one_hot)"""
    after = {k: v.copy() for k, v in before.items()}
    frames = np.full((N, 4 * S, 4 * S, 3), 7, np.uint8)
    oh = np.full((N, S, S, 12), 7, np.uint8)
    for i in sel:
        if i >= upto:
            continue
        rs = np.random.RandomState()
        rs.set_state(('MT19937', before['rng_key'][i], int(before['rng_pos'][i]), 0, 0.0))
        d = int(desired[i]) & 0x1FF
        g, a = M.imagine(before['state_init_grid'][i], before['state_init_agent_rc'][i], before['state_agent_rc'][i], d, rs)
        s = rs.get_state()
        after['rng_key'][i], after['rng_pos'][i] = s[1], s[2]
        frames[i], oh[i] = M.render(g, a), M.one_hot(g, a)
        if commit:
            after['state_goal_grid'][i], after['state_goal_agent_rc'][i], after['state_desired'][i], after['desired_mask'][i] = g, a, d, d
            after['hdr'][i, 6], after['hdr'][i, 7] = d & 0xFF, d >> 8
            if 'desired_goal' in after:
                after['desired_goal'][i] = frames[i]
    return after, frames, oh


def _sample_after(before, sel, upto=N):
    after = {k: v.copy() for k, v in before.items()}
    cells = np.full((N, 9), 999, np.uint16)
    for i in sel:
        if i >= upto:
            continue
        rs = np.random.RandomState()
        rs.set_state(('MT19937', before['rng_key'][i], int(before['rng_pos'][i]), 0, 0.0))
        cells[i] = M.sample_state(S, rs)
        s = rs.get_state()
        after['rng_key'][i], after['rng_pos'][i] = s[1], s[2]
    return after, cells


@pytest.fixture(scope='module')
def case():
    before = _before(True)
    mask = np.zeros(N, np.uint8)
    sel = np.array([0, 3, 9, 10, 11, 17, 30, 33, 36])            # (36: the last, partial chunk of 8; 9, 10, 11: one chunk)
    mask[sel] = [1, 2, 0x80, 0xFF, 1, 1, 1, 1, 1]
    desired = ((np.arange(N) * 37 + 11) % 512 | 0x8000 | ((np.arange(N) % 3) << 10)).astype(np.uint16)      # bits above n_task_list on top
    desired[sel[2]] = 0x1FF
    return before, mask, sel, desired


def _check(case, after, frames, oh, commit=True):
    before, mask, sel, desired = case
    blank_f, blank_o = np.full_like(frames, 7), np.full_like(oh, 7)
    check_masked_call('imagine', before, after, mask, desired=desired, commit=commit, frames=frames, out_before=blank_f)
    check_masked_call('imagine', before, after, mask, desired=desired, commit=commit, one_hot=oh, out_before=blank_o)


def test_snapshots_built_from_the_model_pass(case):
    before, mask, sel, desired = case
    for commit in (False, True):
        after, frames, oh = _imagine_after(before, sel, desired, commit)
        _check(case, after, frames, oh, commit)
    own = before['state_desired']
    after, frames, oh = _imagine_after(before, np.arange(N), own, True)
    assert np.array_equal(check_masked_call('imagine', before, after, None, commit=True, one_hot=oh), np.arange(N))
    after, cells = _sample_after(before, sel)
    rows = check_masked_call('sample', before, after, mask, cells=cells, out_before=np.full((N, 9), 999, np.uint16))
    assert np.array_equal(rows, sel)
    assert len(untouched(before, after, mask)) == N - len(sel)
    st = {k: v for k, v in before.items() if not k.startswith(('observation', 'desired_goal', 'init_observation'))}       # state mode: no frame arrays
    after, frames, oh = _imagine_after(st, sel, desired, True)
    check_masked_call('imagine', st, after, mask, desired=desired, commit=True, one_hot=oh)


def test_nothing_to_compare_is_refused(case):
    before, mask, sel, desired = case
    zero = np.zeros(N, np.uint8)
    after, frames, oh = _imagine_after(before, [], desired, False)
    with pytest.raises(ValueError, match='nothing selected'):
        check_masked_call('imagine', before, after, zero, desired=desired, one_hot=oh)
    assert len(check_masked_call('imagine', before, after, zero, desired=desired, one_hot=oh, out_before=np.full_like(oh, 7), allow_empty=True)) == 0
    with pytest.raises(ValueError, match='no output array'):
        check_masked_call('imagine', before, after, mask, desired=desired)
    with pytest.raises(ValueError, match='every env is selected'):
        untouched(before, after, np.ones(N, np.uint8))
    with pytest.raises(ValueError):
        check_masked_call('imagine', before, after, mask[:-1], one_hot=oh)
    after['rng_pos'][5] += 1                                    # an all-zero mask that moved a stream
    with pytest.raises(AssertionError, match=r'rng_pos .*\[5\]'):
        check_masked_call('imagine', before, after, zero, desired=desired, one_hot=oh, allow_empty=True)


_SELECTED = [('frames', 'frames', (2, 1, 0)), ('one_hot', 'one_hot output|goal grid|goal agent', (2, 3, 8)), ('rng_key', 'rng_key', (600,)), ('rng_pos', 'rng_pos', ()),
             ('state_goal_grid', 'state_goal_grid', (4, 4)), ('state_goal_agent_rc', 'state_goal_agent_rc', (1,)), ('state_desired', 'state_desired', ()),
             ('desired_mask', 'desired_mask', ()), ('hdr', 'hdr', (6,)), ('hdr', 'hdr', (7,)), ('desired_goal', 'desired_goal', (0, 0, 2)),
             # what a relabel must NOT move in a selected row
             ('hdr', 'hdr', (5,)), ('state_grid', 'state_grid', (0, 0)), ('state_step_num', 'state_step_num', ()), ('state_achieved', 'state_achieved', ()),
             ('observation', 'observation', (3, 3, 1)), ('init_observation', 'init_observation', (3, 3, 1)), ('reward', 'reward', ()), ('slot_pos', 'slot_pos', (2,)),
             ('achieved_mask', 'achieved_mask', ()), ('episode_length', 'episode_length', ()), ('state_init_grid', 'state_init_grid', (1, 1))]


@pytest.mark.parametrize('env', [10, 36])
@pytest.mark.parametrize('what,named,at', _SELECTED)
def test_one_wrong_element_in_a_selected_row_fails_and_is_named(case, what, named, at, env):
    before, mask, sel, desired = case
    after, frames, oh = _imagine_after(before, sel, desired, True)
    target = {'frames': frames, 'one_hot': oh}.get(what, after.get(what))
    target[(env,) + at] ^= 1
    with pytest.raises(AssertionError, match=r'(%s) differs .*first \[%d\]' % (named, env)):
        _check(case, after, frames, oh)


@pytest.mark.parametrize('what', ['frames', 'one_hot', 'rng_key', 'rng_pos', 'state_goal_grid', 'state_desired', 'desired_mask', 'hdr', 'desired_goal', 'observation', 'done',
                                  'episode_return', 'state_ep_no', 'state_hold'])
def test_one_wrong_element_in_an_unselected_row_fails(case, what):
    before, mask, sel, desired = case
    after, frames, oh = _imagine_after(before, sel, desired, True)
    target = {'frames': frames, 'one_hot': oh}.get(what, after.get(what))
    target[12:13].reshape(-1)[-1:] ^= 1                            # (env 12: in the chunk of 9, 10, 11, not selected)
    with pytest.raises(AssertionError, match=r'differs .*first \[12\]'):
        _check(case, after, frames, oh)
    after, cells = _sample_after(before, sel)
    if what in after:
        after[what][12:13].reshape(-1)[-1:] ^= 1
        with pytest.raises(AssertionError, match=r'differs .*first \[12\]'):
            check_masked_call('sample', before, after, mask, cells=cells)
        with pytest.raises(AssertionError, match=r'differs .*first \[12\]'):
            untouched(before, after, mask)


def test_counters_that_moved_fail(case):
    before, mask, sel, desired = case
    after, frames, oh = _imagine_after(before, sel, desired, True)
    after['counters'][5] += 1
    with pytest.raises(AssertionError, match='counters changed'):
        _check(case, after, frames, oh)


def test_a_kernel_that_stops_before_the_last_partial_chunk_fails(case):
    before, mask, sel, desired = case
    assert N // EPB * EPB == 32 < sel[-2] < sel[-1]
    for commit in (False, True):
        after, frames, oh = _imagine_after(before, sel, desired, commit, upto=N // EPB * EPB)
        with pytest.raises(AssertionError, match=r'differs .* at 2 envs, first \[33, 36\]'):
            _check(case, after, frames, oh, commit)
    after, cells = _sample_after(before, sel, upto=N // EPB * EPB)
    with pytest.raises(AssertionError, match=r'cells differs .*first \[33, 36\]'):
        check_masked_call('sample', before, after, mask, cells=cells)


def test_two_envs_results_swapped_within_a_chunk_fail(case):
    before, mask, sel, desired = case
    after, frames, oh = _imagine_after(before, sel, desired, True)
    for arr in (frames, oh, after['rng_key'], after['rng_pos'], after['state_goal_grid'], after['state_goal_agent_rc'], after['desired_goal']):
        arr[[9, 10]] = arr[[10, 9]]
    with pytest.raises(AssertionError, match=r'differs .*first \[9, 10\]'):
        _check(case, after, frames, oh)
    after, cells = _sample_after(before, sel)
    cells[[9, 10]] = cells[[10, 9]]                              # only the output rows swapped: the streams are right
    with pytest.raises(AssertionError, match=r'cells differs .*first \[9, 10\]'):
        check_masked_call('sample', before, after, mask, cells=cells)


def test_desired_bits_above_the_task_list_and_odd_mask_bytes(case):
    """the checker models what the kernel reads: any non-zero byte selects, and of a desired word only the bits below n_task_list count"""
    before, mask, sel, desired = case
    after, frames, oh = _imagine_after(before, sel, desired & 0x1FF, True)
    check_masked_call('imagine', before, after, mask != 0, desired=desired, commit=True, one_hot=oh)
    after['desired_mask'][sel[0]] = desired[sel[0]]              # the unmasked word committed
    with pytest.raises(AssertionError, match=r'desired_mask differs .*first \[0\]'):
        check_masked_call('imagine', before, after, mask, desired=desired, commit=True, one_hot=oh)


def test_the_launch_rule():
    """cwh_masked_launch (cw_host.h: what the masked and snapshot launchers call) as DESIGN.md 5.1 states it, at the figures tests/test_masked_shapes.py asserts
    on 256 CUs -- and the C++ rule equal to masked_check.masked_launch, the copy the GPU tests compute their expectations with"""
    assert [masked_launch(n, 256, 1) for n in (509, 2053, 4099, 8209, 16411, 20011)] == \
        [(4, 128, 128), (8, 257, 256), (16, 257, 256), (32, 257, 256), (64, 257, 256), (64, 313, 256)]
    assert masked_launch(65536, 256)[:2] == (64, 1024) and masked_launch(16384, 256)[0] == 16 and masked_launch(700, 256)[0] == 4
    assert [masked_launch(n, 256)[0] for n in (1, 2, 3, 5, 63, 64, 65)] == [4] * 7
    assert masked_launch(1, 256) == (4, 1, 1) and masked_launch(37, 1, 1) == (64, 1, 1)
    lib = host_lib()[1]
    blocks = C.c_int(0)
    sizes = sorted(set(range(1, 70001, 97)) | {p + d for k in range(18) for p in [2 ** k] for d in (-1, 0, 1) if p + d >= 1})
    assert sizes[0] == 1 and 131073 in sizes and len(sizes) > 750
    for n_cu in (1, 8, 256, 304):
        for reset_blocks in (1, 4, 16):
            for n in sizes:
                epb = lib.cwh_masked_launch_of(n, n_cu, reset_blocks, C.byref(blocks))
                want = masked_launch(n, n_cu, reset_blocks)
                assert (epb, blocks.value) == (want[0], want[2]), (n, n_cu, reset_blocks, epb, blocks.value, want)
                assert lib.cwh_reset_grid_of(want[1] * 4, n_cu, reset_blocks) == want[2]       # (the grid of that many chunks, four waves each)
    # the reset-shaped grid on its own (cw_reset_kernel, cw_refill_kernel, cw_pool_kernel: one wave per env): ceil(jobs / 4), n_cu * reset_blocks at most, 1 at least
    assert [lib.cwh_reset_grid_of(j, 256, 4) for j in (0, 1, 4, 5, 4096, 4097, 65536)] == [1, 1, 1, 2, 1024, 1024, 1024]
    assert lib.cwh_reset_grid_of(4093, 256, 4) == 1024 and lib.cwh_reset_grid_of(4092, 256, 4) == 1023 and lib.cwh_reset_grid_of(2 ** 27, 304, 16) == 4864


def test_the_envs_per_wave_rule():
    """cwh_envs_per_wave (cw_host.h: what the step and rollout launchers call): `most` envs per wave, halved down to 8 while the waves would number under
    1 024 -- the widths 64 / 32 / 16 / 8 tests/test_launch_shapes.py runs, at the N where each begins"""
    f = host_lib()[1].cwh_envs_per_wave_of
    for width in (64, 32, 16):                                                     # ceil(N / width) reaches 1 024 at N = 1 023 * width + 1
        assert f(1023 * width + 1, 64) == width and f(1023 * width, 64) == width // 2, width
    assert (f(65473, 64), f(32737, 64), f(16369, 64), f(16368, 64)) == (64, 32, 16, 8)
    assert [f(n, 64) for n in (1, 7, 8, 8192)] == [8] * 4 and f(65536, 64) == 64 and f(2 ** 27, 64) == 64
    for most in (32, 16):                                                          # CW_TUNE_STEP_ENVS_PER_WAVE caps the width, the thresholds below it stay
        assert f(2 ** 20, most) == most and f(1023 * most + 1, most) == most and f(1023 * most, most) == most // 2
    assert [f(n, 8) for n in (1, 8193, 2 ** 20)] == [8] * 3
