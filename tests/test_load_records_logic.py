"""CPU tier: the checker of the record loads checked itself (tests/load_records_check.py: check_load_records).  The snapshots come from the CPU model
(tests/load_records_model.py, dressed as masked_check.take() by engine_model.as_take): a right `after` passes, and each deliberately wrong one -- a loaded
env left unchanged, the menu byte taken from the record, a start or goal frame touched, an unselected env changed, a wrong counters[6], a wrong status
byte, reward written -- is caught.  No GPU."""
import numpy as np
import pytest

from engine_model import as_take
from engines import N1
from load_records_check import BAD_INDEX, LOADED, NO_PART, REFUSED, SKIPPED, check_load_records, mutated
from load_records_model import load_src, model_for
from oracle_replay import np_states

S = 5


@pytest.fixture(scope='module')
def case():
    """-> (before, after, hdr, slot_pos, src, status): a load on the dirty-cell ray engine's model, nine steps after the records were taken"""
    keys, pos = np_states(N1, 41000)
    model, _ = model_for('dirty_ray_auto', S, keys, pos)
    model.reset()
    rs = np.random.RandomState(2)
    model.steps(rs.randint(0, 6, (6, N1)))
    hdr, slot_pos = model.records(flags=2)
    hdr[:, 3] = 9                                                 # a menu byte no env has
    hdr[0], slot_pos[0] = mutated('code 9', S)
    model.steps(rs.randint(0, 6, (9, N1)))
    before = as_take(model, pixels=True)
    src = load_src(rs, N1, N1)
    src[np.flatnonzero(src >= 0)[0]] = 0                          # (the refused record is named)
    status = model.load_records(hdr, slot_pos, src)
    after = as_take(model, pixels=True)
    good = np.flatnonzero(status == LOADED)
    after['hdr'][good] = hdr[src[good]]
    after['hdr'][good, 3] = before['hdr'][good, 3]
    after['slot_pos'][good] = slot_pos[src[good]].view(np.int16)
    return before, after, hdr, slot_pos, src, status


def _copy(snap):
    return {k: v.copy() for k, v in snap.items()}


def test_a_right_load_passes_and_every_status_occurs(case):
    before, after, hdr, slot_pos, src, status = case
    want = check_load_records(before, after, hdr, slot_pos, src, status=status)
    assert np.array_equal(want, status)
    assert {int(s) for s in status} == {NO_PART, LOADED, BAD_INDEX, REFUSED} and (status == LOADED).sum() >= 40
    assert after['counters'][SKIPPED] == before['counters'][SKIPPED] + (status >= BAD_INDEX).sum() >= before['counters'][SKIPPED] + 3
    good = np.flatnonzero(status == LOADED)
    assert not np.array_equal(after['observation'][good], before['observation'][good])       # (the load changed what the checker compares)
    assert not np.array_equal(after['state_grid'][good], before['state_grid'][good])


def _wrong(case, edit, match):
    before, after, hdr, slot_pos, src, status = case
    bad, st = _copy(after), status.copy()
    edit(before, bad, st, np.flatnonzero(status == LOADED), np.flatnonzero(status != LOADED))
    with pytest.raises(AssertionError, match=match):
        check_load_records(before, bad, hdr, slot_pos, src, status=st)


def test_a_loaded_env_left_unchanged_is_caught(case):
    def edit(before, bad, st, good, rest):
        for k in bad:
            if k != 'counters':
                bad[k][good[3]] = before[k][good[3]]
    _wrong(case, edit, 'after a record load')


def test_the_menu_byte_taken_from_the_record_is_caught(case):
    def edit(before, bad, st, good, rest):
        bad['hdr'][good[1], 3] = 9
    _wrong(case, edit, 'after a record load: hdr')


@pytest.mark.parametrize('frame', ['init_observation', 'desired_goal'])
def test_a_touched_start_or_goal_frame_is_caught(case, frame):
    def edit(before, bad, st, good, rest):
        bad[frame][good[0], 0, 0, 0] ^= 1
    _wrong(case, edit, 'after a record load: ' + frame)


def test_an_unselected_env_changed_is_caught(case):
    def edit(before, bad, st, good, rest):
        bad['slot_pos'][rest[0], 2] += 1
    _wrong(case, edit, 'after a record load: slot_pos')

    def edit_refused(before, bad, st, good, rest):
        i = np.flatnonzero(st == REFUSED)[0]
        bad['observation'][i, 1, 1, 1] ^= 1
    _wrong(case, edit_refused, 'after a record load: observation')


@pytest.mark.parametrize('delta', [-1, 1, -3])
def test_a_wrong_count_of_skipped_envs_is_caught(case, delta):
    def edit(before, bad, st, good, rest):
        bad['counters'][SKIPPED] += delta
    _wrong(case, edit, 'counters after a record load')


def test_another_counter_moved_is_caught(case):
    def edit(before, bad, st, good, rest):
        bad['counters'][0] += 1
    _wrong(case, edit, 'counters after a record load')


@pytest.mark.parametrize('which', [NO_PART, LOADED, BAD_INDEX, REFUSED])
def test_a_wrong_status_byte_is_caught(case, which):
    def edit(before, bad, st, good, rest):
        i = np.flatnonzero(st == which)[0]
        st[i] = (which + 1) % 4
    _wrong(case, edit, 'status')


def test_reward_written_is_caught(case):
    def edit(before, bad, st, good, rest):
        bad['reward'][good[2]] += 1
    _wrong(case, edit, 'after a record load: reward')


def test_nothing_loaded_is_refused_unless_asked_for(case):
    before, _, hdr, slot_pos, _, _ = case
    src = np.full(N1, -1, np.int32)
    with pytest.raises(ValueError):
        check_load_records(before, before, hdr, slot_pos, src)
    assert (check_load_records(before, before, hdr, slot_pos, src, allow_empty=True) == NO_PART).all()
    with pytest.raises(ValueError):
        check_load_records(before, before, hdr[:5], slot_pos[:5], None)
