"""CPU tier: the two table fixtures (tests/golden/table5_ray.npz, walls8_ray_alt.npz: what the reference classes answered on state_tables' own tables, written
by tools/gen_table_golden.py), their loader and the row comparator of tests/state_tables.py.  What the tables exercise is counted here from the REFERENCE's
rows alone -- neither the oracle nor the engine is called -- and the comparator has to name the row of one flipped byte in every stored column.  No GPU."""
import json
import os

import numpy as np
import pytest

from state_tables import (DYNAMICS, GOLDEN, OUTCOME, TABLE_FIXTURES, first_difference, input_crcs, load_table_fixture, same_table, successor_grids)

CAP = 128 * 1024
COLUMNS = ('desired',) + DYNAMICS + OUTCOME
FRAME_COLUMNS = ('crc_ray', 'crc_alt')


@pytest.fixture(scope='module')
def fixtures():
    return {name: load_table_fixture(name) for name in TABLE_FIXTURES}


def _raw(name):
    z = np.load(os.path.join(GOLDEN, name + '.npz'))
    return {k: z[k] for k in z.files}


def _changed(fx):
    grid, _, agent, hold, _ = fx['table']
    return (fx['agent'] != agent[None]).any(axis=-1) | (fx['hold'] != hold[None]) | (fx['grid'] != grid[None]).any(axis=(-1, -2))


def test_the_files_are_small_and_describe_their_tables(fixtures):
    for name, fx in fixtures.items():
        assert os.path.getsize(os.path.join(GOLDEN, name + '.npz')) < CAP, name
        raw = _raw(name)
        stored = {'desired': np.uint16, 'achieved': np.uint16, 'agent': np.uint8, 'hold': np.uint8, 'own': np.uint8, 'new': np.uint8, 'reward': np.int8, 'done': np.uint8}
        assert all(raw[k].dtype == dt for k, dt in stored.items()), name
        assert fx['meta']['env'] == 'CraftingWorldEnvRay' and fx['meta']['input_crc'] == input_crcs(fx['table'])
        assert fx['n'] == len(fx['table'][3]) == {'table5_ray': 18816, 'walls8_ray_alt': 1296}[name]
        assert fx['step_nums'] == {'table5_ray': [3, 8], 'walls8_ray_alt': [3]}[name] and fx['max_steps'] == 9
        assert set(np.unique(fx['reward'])) == {-1, 9} and set(np.unique(fx['done'])) == {0, 1}
        assert ((fx['desired'] >= 1) & (fx['desired'] < 512)).all() and (fx['achieved'] < 512).all() and fx['hold'].max() == 3
        assert ((fx['reward'] == 9) <= (fx['done'] == 1)).all()                     # a success ends the episode under either rule
    raw = _raw('walls8_ray_alt')
    assert all(raw[k].dtype == np.uint32 and raw[k].shape == (6, 1296) for k in FRAME_COLUMNS)
    assert not set(FRAME_COLUMNS) & set(fixtures['table5_ray'])


def test_a_step_changes_at_most_the_start_cell_and_the_end_cell(fixtures):
    """the successor grids are the state's grid but for own and new; an unchanged row leaves both codes as they were, a move leaves the start cell as it was"""
    for name, fx in fixtures.items():
        grid, _, agent, hold, _ = fx['table']
        j = np.arange(fx['n'])
        was_own = grid[j, agent[:, 0], agent[:, 1]]
        for a in range(6):
            end = fx['agent'][a]
            assert (np.abs(end - agent).sum(axis=1) <= 1).all(), (name, a)          # at most one cell away
            if a >= 4:
                assert (end == agent).all() and (fx['own'][a] == fx['new'][a]).all(), (name, a)
            else:
                moved = (end != agent).any(axis=1)
                assert (fx['own'][a][moved] == was_own[moved]).all() and (fx['hold'][a] == hold).all(), (name, a)
        still = ~_changed(fx)
        assert (fx['new'][still] == np.broadcast_to(was_own, (6, fx['n']))[still]).all(), name


def test_a_table_rebuilt_differently_is_refused(tmp_path):
    raw = _raw('walls8_ray_alt')
    meta = json.loads(bytes(raw['meta']).decode())
    meta['input_crc']['init_grid'] ^= 1
    raw['meta'] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = str(tmp_path / 'walls8_ray_alt.npz')
    np.savez(path, **raw)
    with pytest.raises(ValueError, match='not the one the fixture was recorded on'):
        load_table_fixture('walls8_ray_alt', path)
    with pytest.raises(ValueError):
        load_table_fixture('walls9')


def test_what_the_local_table_exercises_by_the_references_rows(fixtures):
    """the floors test_expand.test_the_whole_local_transition_table asserts from the oracle's values, here from the reference's"""
    fx = fixtures['table5_ray']
    ach = fx['table'][4]
    gained, lost = fx['achieved'] & ~ach, ach & ~fx['achieved']
    gains = [int(((gained >> b) & 1).sum()) for b in range(9)]
    losses = [int(((lost >> b) & 1).sum()) for b in range(5, 9)]
    changed = _changed(fx)
    success = (fx['reward'] == fx['max_steps']).sum(axis=(2, 3))
    timeout_only = ((fx['done'] == 1) & (fx['reward'] != fx['max_steps'])).sum(axis=(2, 3))
    print('gains', gains, 'losses of bits 5..8', losses, 'successes [rule, step_num]', success.tolist(), 'changed', int(changed.sum()), 'unchanged',
          int((~changed).sum()), 'done by time-out alone [rule, step_num]', timeout_only.tolist())
    assert min(gains) >= 100 and min(losses) >= 400 and success.min() >= 10000
    assert changed.sum() >= 50000 and (~changed).sum() >= 50000
    assert fx['step_nums'][1] == fx['max_steps'] - 1 and timeout_only[:, 1].min() >= 80000 and (timeout_only[:, 0] == 0).all()
    assert (fx['done'][:, 1] == 1).all()
    # an unchanged row pays -1 whatever the masks say (ray.py:362-363), and the rules differ somewhere
    assert (fx['reward'][:, :, ~changed] == -1).all() and (fx['reward'][0] != fx['reward'][1]).any()


def test_what_the_wall_table_exercises_by_the_references_rows(fixtures):
    fx = fixtures['walls8_ray_alt']
    _, _, agent, _, ach = fx['table']
    changed = _changed(fx)
    blocked = [int((~changed[a]).sum()) for a in range(4)]
    gained = fx['achieved'] & ~ach
    print('blocked moves', blocked, 'changed', int(changed.sum()), 'gains', [int(((gained >> b) & 1).sum()) for b in range(9)])
    assert min(blocked) >= 144 * 3                                   # every move runs into its wall at three of the nine anchors at least
    for a, (axis, edge) in enumerate([(0, 0), (1, 7), (0, 7), (1, 0)]):
        at_wall = agent[:, axis] == edge
        assert at_wall.sum() == 144 * 3 and not changed[a][at_wall].any() and (fx['agent'][a][at_wall] == agent[at_wall]).all()
    assert changed[4].sum() >= 20 and changed[5].sum() >= 20 and all(((gained >> b) & 1).any() for b in range(9))
    assert len(np.unique(fx['crc_ray'])) >= 1296 and len(np.unique(fx['crc_alt'])) >= 1296
    still = ~changed
    for k in FRAME_COLUMNS:                                              # an unchanged row keeps its frame: the same for every such action of a state
        first = np.where(still, fx[k], 0).max(axis=0)
        assert (np.where(still, fx[k], first[None]) == first[None]).all(), k


@pytest.mark.parametrize('name,column', [(n, c) for n in TABLE_FIXTURES for c in COLUMNS + (FRAME_COLUMNS if n == 'walls8_ray_alt' else ())])
def test_the_comparator_names_the_row_of_one_flipped_byte(fixtures, name, column):
    """a copy of the fixture's column with one byte flipped: same_table refuses it and names the state, the action, the field and the table's case"""
    fx = fixtures[name]
    raw = _raw(name)[column]
    same_table({column: fx[column]}, {column: raw.astype(np.int64)}, fx['cases'])          # (the copy itself passes)
    for where in (0.0, 0.37, 0.999):
        bad = raw.copy()
        k = int(where * (bad.nbytes - 1))
        bad.view(np.uint8).reshape(-1)[k] ^= 0x04
        idx = np.unravel_index(k // bad.itemsize, bad.shape)
        axis = bad.shape.index(fx['n'])
        state, action = int(idx[axis]), (int(idx[axis - 1]) if axis else None)
        d = first_difference(column, fx[column], bad.astype(np.int64), fx['cases'])
        assert d is not None and d[:4] == (state, action, column, fx['cases'][state])
        assert d[4] == int(bad[idx]) and d[5] == int(raw[idx]) and d[4] != d[5]
        with pytest.raises(AssertionError) as err:
            same_table({column: fx[column]}, {column: bad.astype(np.int64)}, fx['cases'])
        msg = str(err.value)
        assert '%s differs first at state %d, action %s:' % (column, state, action) in msg and repr(fx['cases'][state]) in msg
        if column == 'new':                                               # ... and so do the successor grids built from it, in the cell the agent ends on
            g = successor_grids(fx['table'][0], fx['table'][2], fx['agent'], fx['own'], bad.astype(np.int64))
            dg = first_difference('grid', fx['grid'], g, fx['cases'])
            assert dg is not None and dg[:2] == (state, action)


def test_the_comparator_refuses_what_it_cannot_place(fixtures):
    fx = fixtures['walls8_ray_alt']
    with pytest.raises(ValueError):
        first_difference('hold', fx['hold'], fx['hold'][:, :-1], fx['cases'])
    with pytest.raises(ValueError):
        first_difference('hold', fx['hold'][:, :5], fx['hold'][:, :5], fx['cases'])
    assert first_difference('hold', fx['hold'], fx['hold'].copy(), fx['cases']) is None
