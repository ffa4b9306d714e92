"""CPU tier: tests/refit_check.py itself -- the numpy model of cw_shoot_refit against the library's own cwh_refit_weight_of, the elite rule on columns worked
out by hand, the checker against planted faults (each caught at its place), and, from the model alone, that every tie-bearing input the GPU tier uses has
a state whose threshold value is shared by a chosen and an unchosen sample: otherwise the tie rule would not be tested there."""
import numpy as np
import pytest

import refit_check as rc
from hostlib import host_lib
from shoot_check import model_actions

GPU_M, GPU_K = (1, 65, 600), (1, 2, 5, 9, 17, 63, 64, 65, 100, 129, 1000)       # tests/test_refit.py's selection shapes


def gpu_elites(K):
    return sorted({1, -(-K // 3), K})


def test_the_weight_formula_against_the_library():
    """10^5 inputs: smooth = 0 included, the clamp at 65 535 reached, the largest arguments the entry point accepts (no wrap in uint32)"""
    _, lib = host_lib()
    rng = np.random.RandomState(5)
    n = 100000
    smooth = rng.randint(0, 65536, n)
    gain = rng.randint(1, 65536, n)
    count = rng.randint(0, 65537, n)
    smooth[:20000] = 0
    gain[20000:60000] = rng.randint(1, 40, 40000)
    count[20000:60000] = rng.randint(0, 200, 40000)
    smooth[20000:40000] = rng.randint(0, 3, 20000)
    smooth[-3:], gain[-3:], count[-3:] = (65535, 0, 65535), (65535, 1, 1), (65536, 65535, 0)
    want = rc.weight(smooth, gain, count)
    got = np.array([lib.cwh_refit_weight_of(int(s), int(g), int(c)) for s, g, c in zip(smooth, gain, count)])
    assert np.array_equal(got, want)
    assert (want == 65535).sum() > 1000 and (want < 65535).sum() > 20000 and (want[smooth == 0] < 65535).any() and want.min() == 0
    assert [lib.cwh_refit_weight_of(*a) for a in ((0, 1, 0), (1, 1, 0), (0, 1, 65535), (0, 1, 65536), (1, 1, 65534), (65535, 65535, 65536), (3, 7, 11))] == \
        [0, 1, 65535, 65535, 65535, 65535, 80]


def test_the_elite_rule_by_hand():
    ret = np.array([[5, 1, 0, 3], [5, 2, 0, 3], [7, 2, 0, -9], [5, 2, 0, 3], [9, 0, 0, 2 ** 31 - 1], [5, 2, 0, -2 ** 31]], np.int32)      # [K = 6, M = 4]
    e, v = rc.expected_elites(ret, 3)
    assert e.T.tolist() == [[0, 2, 4], [1, 2, 3], [0, 1, 2], [0, 1, 4]] and v.tolist() == [5, 2, 0, 3]
    assert rc.split_ties(ret, 3).tolist() == [True, True, True, True]
    e, v = rc.expected_elites(ret, 1)
    assert e.tolist() == [[4, 1, 0, 4]] and v.tolist() == [9, 2, 0, 2 ** 31 - 1] and rc.split_ties(ret, 1).tolist() == [False, True, True, False]
    e, v = rc.expected_elites(ret, 6)
    assert (e == np.arange(6)[:, None]).all() and v.tolist() == [5, 0, 0, -2 ** 31] and not rc.split_ties(ret, 6).any()
    e, v = rc.expected_elites(ret, 2)
    assert e.T.tolist() == [[2, 4], [1, 2], [0, 1], [0, 4]] and rc.split_ties(ret, 2).tolist() == [False, True, True, True]


def test_the_counts_are_the_elites_drawn_actions():
    K, M, E, T, seed = 9, 7, 4, 5, 2 ** 64 - 3
    rng = np.random.RandomState(3)
    ret = rng.randint(-3, 4, (K, M)).astype(np.int32)
    w_in = rng.randint(0, 4, (T, 6, M)) * rng.randint(0, 30000, (T, 6, M))
    for weights in (None, w_in):
        want = rc.expected_refit(ret, E, T, seed, weights, smooth=2, gain=3)
        acts = model_actions(seed, M, K, T, weights)                                     # every sample's actions [T, K, M]
        for j in range(M):
            for t in range(T):
                hist = np.bincount(acts[t, want['elites'][:, j], j], minlength=6)
                assert hist.tolist() == want['counts'][t, :, j].tolist()
                assert (2 + 3 * hist).tolist() == want['weights'][t, :, j].tolist()
    assert not np.array_equal(rc.expected_refit(ret, E, T, seed, None)['counts'], rc.expected_refit(ret, E, T, seed, w_in)['counts'])


# ---------------------------------------------------------------------------------------------------------------- the checker and planted faults
K, M, E, T, SEED, N_ENVS = 12, 40, 4, 6, 77, 9


def a_call(in_place=False, weighted=True, smooth=1, gain=1, e=E):
    """a correct call on the CPU: everything check_refit takes"""
    rng = np.random.RandomState(11)
    ret = rng.randint(-2, 3, (K, M)).astype(np.int32)
    assert rc.split_ties(ret, e).sum() >= M // 2
    w_in = rng.randint(0, 500, (T, 6, M)).astype(np.uint16) if weighted else None
    env_of = rng.randint(0, N_ENVS, M).astype(np.int32)
    env_of[[3, 17]] = -1, -5
    env_of[[8, 30]] = N_ENVS, 2 ** 31 - 1
    part = rc.takes_part(env_of, N_ENVS, M)
    want = rc.expected_refit(ret, e, T, SEED, w_in, smooth, gain)
    before = dict(elites=np.full((e, M), -99, np.int32), weights=w_in.copy() if in_place else np.full((T, 6, M), 0xABCD, np.uint16),
                  elite_min=np.full(M, -98, np.int32))
    after = {f: np.where(part, want[f], before[f]).astype(before[f].dtype) for f in rc.FIELDS}
    return dict(ret_before=ret, ret_after=ret.copy(), weights_in_before=w_in, weights_in_after=None if w_in is None else w_in.copy(), env_of=env_of,
                num_envs=N_ENVS, E=e, T=T, seed=SEED, smooth=smooth, gain=gain, before=before, after=after, in_place=in_place), part, want


@pytest.mark.parametrize('in_place, weighted', [(False, False), (False, True), (True, True)])
def test_a_correct_call_passes(in_place, weighted):
    call, part, _ = a_call(in_place, weighted)
    assert rc.check_refit(**call) == (M - 4, 4) and part.sum() == M - 4
    del call['before']['weights'], call['after']['weights']                              # selection only
    assert rc.check_refit(**call) == (M - 4, 4)


def split_state(call, part):
    j = int(np.flatnonzero(rc.split_ties(call['ret_before'], call['E']) & part)[0])
    return j


def test_a_tie_given_to_the_larger_sample_is_caught():
    call, part, want = a_call()
    j = split_state(call, part)
    col, v = call['ret_before'][:, j], want['elite_min'][j]
    chosen = [k for k in want['elites'][:, j] if col[k] == v]
    spare = [k for k in range(K) if col[k] == v and k not in want['elites'][:, j]]
    e = sorted(set(want['elites'][:, j]) - {chosen[-1]} | {spare[-1]})                    # the same returns, a larger sample
    assert sorted(col[e]) == sorted(col[want['elites'][:, j]])
    call['after']['elites'][:, j] = e
    with pytest.raises(AssertionError, match=r'elites\[\d+, %d\] of a state that takes part' % j):
        rc.check_refit(**call)


def test_elites_not_ascending_are_caught():
    call, part, want = a_call()
    j = int(np.flatnonzero(part)[5])
    call['after']['elites'][:, j] = want['elites'][::-1, j]
    with pytest.raises(AssertionError, match=r'elites\[0..1, %d\] not ascending' % j):
        rc.check_refit(**call)


@pytest.mark.parametrize('off', [-1, 1])
def test_an_elite_count_off_by_one_is_caught(off):
    call, part, _ = a_call()
    other = rc.expected_refit(call['ret_before'], E + off, T, SEED, call['weights_in_before'])
    rows = min(E, E + off)
    call['after']['elites'][:rows] = np.where(part, other['elites'][:rows], call['after']['elites'][:rows])
    with pytest.raises(AssertionError, match='elites'):
        rc.check_refit(**call)
    call, part, _ = a_call()                                                              # ... or only in what is counted
    call['after']['weights'] = np.where(part, other['weights'], call['after']['weights']).astype(np.uint16)
    with pytest.raises(AssertionError, match=r'weights\[\d+, \d+, \d+\] of a state that takes part'):
        rc.check_refit(**call)
    call, part, _ = a_call()
    call['after']['elite_min'] = np.where(part, other['elite_min'], call['after']['elite_min']).astype(np.int32)
    if (other['elite_min'] != rc.expected_elites(call['ret_before'], E)[1])[part].any():
        with pytest.raises(AssertionError, match='elite_min'):
            rc.check_refit(**call)


def test_counts_under_uniform_actions_are_caught_when_weights_were_given():
    call, part, _ = a_call()
    uniform = rc.expected_refit(call['ret_before'], E, T, SEED, None)
    call['after']['weights'] = np.where(part, uniform['weights'], call['after']['weights']).astype(np.uint16)
    with pytest.raises(AssertionError, match=r'weights\[\d+, \d+, \d+\] of a state that takes part'):
        rc.check_refit(**call)


def test_a_missing_clamp_is_caught():
    call, part, want = a_call(gain=30000)
    assert (want['weights'] == 65535).any() and (want['weights'] < 65535).any()
    wrapped = (1 + 30000 * want['counts']) & 0xFFFF                                       # what a store of the unclamped sum leaves
    call['after']['weights'] = np.where(part, wrapped, call['after']['weights']).astype(np.uint16)
    with pytest.raises(AssertionError, match=r'weights\[\d+, \d+, \d+\] of a state that takes part: got \d+, expected 65535'):
        rc.check_refit(**call)


@pytest.mark.parametrize('field, at', [('elites', (2, 17)), ('weights', (4, 5, 8)), ('elite_min', (30,)), ('elites', (0, 3))])
def test_a_written_row_of_a_state_that_takes_no_part_is_caught(field, at):
    call, part, want = a_call()
    assert not part[at[-1]]
    call['after'][field][at] = want[field][at] if want[field][at] != call['before'][field][at] else 1
    with pytest.raises(AssertionError, match=r'%s\[%s\] of a state that takes no part was written' % (field, ', '.join(str(i) for i in at))):
        rc.check_refit(**call)


def test_a_written_row_is_caught_in_place_too():
    call, part, want = a_call(in_place=True)
    rc.check_refit(**call)
    call['after']['weights'][1, 2, 3] ^= 1                                                # state 3 takes no part: its weights stay the input's
    with pytest.raises(AssertionError, match=r'weights\[1, 2, 3\] of a state that takes no part was written'):
        rc.check_refit(**call)


def test_a_changed_byte_of_ret_is_caught():
    call, _, _ = a_call()
    call['ret_after'].reshape(-1).view(np.uint8)[5 * M * 4 + 13] ^= 0x40
    with pytest.raises(AssertionError, match=r'ret\[5, 3\] was changed by the call'):
        rc.check_refit(**call)


def test_a_changed_byte_of_weights_in_is_caught_unless_in_place():
    call, _, _ = a_call()
    call['weights_in_after'].reshape(-1).view(np.uint8)[(2 * 6 + 1) * M * 2 + 8] ^= 1
    with pytest.raises(AssertionError, match=r'weights_in\[2, 1, 4\] was changed by a call that is not in place'):
        rc.check_refit(**call)
    call, _, _ = a_call(in_place=True)
    call['weights_in_after'] = None                                                       # (in place there is no such buffer)
    rc.check_refit(**call)


# ---------------------------------------------------------------------------------------------------------------- the GPU tier's inputs
@pytest.mark.parametrize('kind', rc.KINDS)
def test_the_columns_of_the_gpu_tier(kind):
    """from the model alone: every tie-bearing input has a state whose threshold value is held by a chosen and an unchosen sample, whenever E < K leaves
    one unchosen; the permutations have no tie at all; the lane kind puts the chosen and the unchosen holder on every sample position it can"""
    for m in GPU_M:
        for k in GPU_K:
            for e in gpu_elites(k):
                ret = rc.columns(kind, k, m, e)
                assert ret.shape == (k, m) and ret.dtype == np.int32
                split = rc.split_ties(ret, e)
                if kind in rc.TIE_BEARING and k > e:
                    assert split.any(), (kind, m, k, e)
                if kind == 'perm':
                    assert not split.any() and all(len(set(ret[:, j])) == k for j in range(0, m, 7))
                if kind == 'extremes' and m >= 5 and 3 <= e < k:
                    assert {rc.INT32_MIN, 0, rc.INT32_MAX} <= set(rc.expected_elites(ret, e)[1].tolist()), (m, k, e)
                if kind == 'lane' and m >= k > e:
                    elites, v = rc.expected_elites(ret, e)
                    holds, chosen = ret == v[None], np.zeros((k, m), bool)
                    np.put_along_axis(chosen, elites, True, axis=0)
                    assert (holds & chosen).any(axis=1)[:-1].all() and (holds & ~chosen).any(axis=1)[1:].all(), (m, k, e)
    big = rc.columns('two', 4, 65536, 2)
    assert rc.split_ties(big, 2).sum() > 10000


@pytest.mark.parametrize('k', [k for k in GPU_K if k <= 129])
def test_shoots_own_returns_are_heavy_in_ties(k):
    """the sixth kind: the returns shoot() gives simulate_check.recipe(12)'s states at T = 6 (here from the oracle; the GPU tier asserts the same of the
    returns the card gave, whatever K); one state is the first column that has such a tie: refit_check.shoot_columns"""
    from shoot_check import recipe_shots
    ret = recipe_shots(6, k, 3)[2]['ret']
    for m in GPU_M:
        for e in gpu_elites(k):
            if k > e:
                assert rc.split_ties(ret[:, rc.shoot_columns(ret, m, e)], e).any(), (m, k, e)
