"""CPU tier: the checker of the seen tests (tests/seen_check.py) itself, and the claim reach() rests on.  The outputs a correct cw_seen_insert would leave are
synthesised on the CPU from the model and must pass; each planted fault must be caught.  reference_reach -- breadth-first, states merged by key -- equals
brute force over all 6^D action strings by the oracle alone: merging by key loses no shortest solution.  Also here: what the oracle says of the start rows
the reach tests share."""
import numpy as np
import pytest

from records_check import encode
from records_fixtures import N, S, SENT, snap, world
from seen_check import (REACH_MAX_STEPS, REACH_N, REACH_SEEDS, SeenModel, brute_reach, check_seen_call, groups_of, key_of, oracle_starts,
                        reach_reference, reference_reach)

M = 24


def _records():
    """M records: the five envs' states over and over (so keys repeat), menu bytes, step counts and flag bits that must not matter, two rows that take no part"""
    dense, init_grids = world()
    pick = np.arange(M) % N
    sub = {k: v[pick] for k, v in dense.items()}
    sub['step_num'] = np.arange(M) % 7
    sub['flags'] = (sub['flags'] & 2) | (np.arange(M) % 2) | ((np.arange(M) % 3) << 2)
    hdr, pos = encode(sub, menu=np.arange(M) % 4)
    group = np.arange(M, dtype=np.int64) % N
    group[12:] += N * (np.arange(12) % 2)        # the same records in other groups: apart
    group[[3, 20]] = [-1, -9]
    return dense, init_grids, hdr, pos, group


def _correct(group_given=True, calls=1):
    """what `calls` correct calls on the same rows leave: the arguments of check_seen_call for the LAST one, with the model as it stood before it"""
    dense, init_grids, hdr, pos, group = _records()
    g = group if group_given else None
    gg = groups_of(g, M, N)
    keys, part = key_of(hdr, pos, np.where(gg >= 0, gg, 0)), gg >= 0
    engine, model, shadow = snap(dense, init_grids), SeenModel(), SeenModel()
    c0 = np.zeros(3, np.int64)
    for _ in range(calls - 1):
        model.insert(keys, part)
        shadow.insert(keys, part)
    c0[0] = len(shadow)
    fresh, first = shadow.insert(keys, part)
    out = dict(fresh=np.where(part, fresh, SENT).astype(np.uint8), first=first.astype(np.int32))
    out['first'].view(np.uint8).reshape(M, 4)[~part] = SENT
    c1 = c0.copy()
    c1[0] = len(shadow)
    return model, dict(hdr=hdr, slot_pos=pos, group=g, num_envs=N), out, c0, c1, engine, {k: v.copy() for k, v in engine.items()}


def _check(a, **kw):
    return check_seen_call(a[0], a[1], a[2], SENT, a[3], a[4], a[5], a[6], **kw)


@pytest.mark.parametrize('group_given', [True, False])
@pytest.mark.parametrize('calls', [1, 2])
def test_a_correct_call_passes(group_given, calls):
    a = _correct(group_given, calls)
    assert _check(a, exact=True) == 0
    if calls == 2:
        part = groups_of(a[1]['group'], M, N) >= 0
        assert (a[2]['first'][part] == -1).all() and not a[2]['fresh'][part].any()
    else:
        assert a[2]['fresh'].astype(np.int64)[groups_of(a[1]['group'], M, N) >= 0].sum() == len(a[0])
    for f in ('fresh', 'first'):
        b = _correct(group_given, calls)
        assert check_seen_call(b[0], b[1], {f: b[2][f]}, SENT, b[3], b[4], b[5], b[6], exact=True) == 0


def test_the_records_merge_and_stay_apart_as_the_key_says():
    _, _, hdr, pos, group = _records()
    k = key_of(hdr, pos, np.where(group >= 0, group, 0))
    assert (k[0] == k[5]).all() and (k[0] == k[10]).all()          # the same env's state under other menu bytes, step counts and flag bits
    assert (k[0] != k[15]).any() and (k[1:5] != k[0]).any(axis=1).all()


def test_a_duplicate_reported_fresh_without_a_counter_is_caught():
    a = _correct()
    j = int(np.flatnonzero((a[2]['first'] >= 0) & (a[2]['first'] != np.arange(M)) & (a[2]['fresh'] == 0))[0])
    a[2]['first'][j], a[2]['fresh'][j] = j, 1
    with pytest.raises(AssertionError, match='deviate'):
        _check(a)
    a[4][2] += 1                                 # ... and passes once a collision is counted for it -- but never as exact
    b = list(a)
    b[0] = SeenModel()
    assert _check(b) == 1
    b[0] = SeenModel()
    with pytest.raises(AssertionError):
        _check(b, exact=True)


def test_a_seen_key_reported_fresh_without_a_counter_is_caught():
    a = _correct(calls=2)
    j = int(np.flatnonzero(groups_of(a[1]['group'], M, N) >= 0)[2])
    a[2]['first'][j], a[2]['fresh'][j] = j, 1
    with pytest.raises(AssertionError, match='deviate'):
        _check(a)


@pytest.mark.parametrize('field', ['first', 'fresh', 'both'])
def test_a_fresh_key_reported_seen_is_caught_even_when_counters_moved(field):
    a = _correct()
    j = int(np.flatnonzero(a[2]['fresh'] == 1)[1])
    if field != 'fresh':
        a[2]['first'][j] = -1
    if field != 'first':
        a[2]['fresh'][j] = 0
    a[4][1] += 5
    a[4][2] += 5
    with pytest.raises(AssertionError):
        _check(a)


def test_a_touched_sentinel_row_is_caught():
    for f, v in (('first', -1), ('fresh', 0)):
        a = _correct()
        a[2][f][3] = v
        with pytest.raises(AssertionError, match='must not be written'):
            _check(a)


def test_a_wrong_first_is_caught():
    a = _correct()
    j = int(np.flatnonzero((a[2]['first'] >= 0) & (a[2]['first'] != np.arange(M)) & (a[2]['fresh'] == 0))[-1])
    a[2]['first'][j] = (a[2]['first'][j] + 1) % j
    assert a[2]['first'][j] != j
    a[4][2] += 3
    with pytest.raises(AssertionError, match='first differs'):
        _check(a)


def test_a_wrong_size_a_shrunk_counter_and_a_changed_engine_are_caught():
    a = _correct()
    a[4][0] += 1
    with pytest.raises(AssertionError, match='holds'):
        _check(a)
    a = _correct()
    a[3][1] = 2
    with pytest.raises(AssertionError, match='shrank'):
        _check(a)
    a = _correct()
    a[6]['counters'][7] += 1
    with pytest.raises(AssertionError):
        _check(a)
    a = _correct()
    a[1]['group'] = np.full(M, -1)
    with pytest.raises(ValueError):
        _check(a)


# ------------------------------------------------------------------------------------------------------------------------------ reach
@pytest.mark.parametrize('depth', [1, 2, 3, 4])
def test_reference_reach_equals_brute_force(depth):
    """by the oracle alone: the shortest plan found over merged states is the shortest of all 6^D strings (5 x 5; goals 1 .. 4 steps away, and none)"""
    from plan_check import far_goals
    dense, init_grids = world()
    okw = dict(size=(S, S), max_steps=9)
    goal = far_goals(dense, init_grids, np.array([1, 2, 3, 4, 4]), okw)
    assert (goal >= 0).sum() >= 3
    dense = dict(dense, desired=np.where(goal >= 0, goal, dense['desired']), step_num=np.array([0, 0, 0, 0, 6]))
    want = brute_reach(dense, init_grids, depth, okw)
    got = reference_reach(dense, init_grids, depth, okw)
    assert np.array_equal(got['distance'], want), (got['distance'], want)
    if depth == 4:
        assert want.tolist() == [1, -1, -1, 4, -1]    # (row 4: max_steps 9 from step 6 -- the time-out cuts its search at three steps)


@pytest.mark.parametrize('depth', [2, 4])
def test_reference_reach_equals_brute_force_on_fresh_episodes(depth):
    """... and from five start states as reset() leaves them, whose goals the oracle's enumeration finds 2, 3 and 4 steps away, and not within 4"""
    seeds = (4029, 4117, 4066, 4000, 4004)
    dense, init_grids = oracle_starts(seeds, 5, REACH_MAX_STEPS)
    okw = dict(size=(5, 5), max_steps=REACH_MAX_STEPS)
    want = brute_reach(dense, init_grids, depth, okw)
    got = reference_reach(dense, init_grids, depth, okw)
    assert np.array_equal(got['distance'], want), (got['distance'], want)
    assert want.tolist() == ([3, 2, 4, -1, -1] if depth == 4 else [-1, 2, -1, -1, -1])
    assert got['searched_depth'] == depth and len(got['frontier']) == depth and got['frontier'][0] == 5


def test_the_shared_start_rows_are_what_the_reach_tests_need():
    """the oracle alone, depth 10: at least a quarter of the 12 start rows is solved and at least one is not.  5 x 5: 6 solved (2, 3, 5, 6, 9 and 10 steps),
    6 not; 8 x 8: 5 solved (3, 5, 6, 7 and 9 steps), 7 not."""
    want = {5: [5, -1, 9, -1, 6, -1, 10, -1, 3, -1, 2, -1], 8: [7, -1, 9, -1, 5, -1, 6, -1, 3, -1, -1, -1]}
    for size in (5, 8):
        assert len(REACH_SEEDS[size]) == REACH_N
        dense, _, ref = reach_reference(size, 10)
        assert dense['flags'].tolist() == [1] * REACH_N and (dense['step_num'] == 0).all()
        d = ref['distance']
        assert d.tolist() == want[size]
        assert (d >= 0).sum() * 4 >= REACH_N and (d < 0).any()
        assert oracle_starts(REACH_SEEDS[size], size, REACH_MAX_STEPS)[0] is dense
