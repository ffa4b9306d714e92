"""The numpy model of imagine_obs() (tests/imagine_model.py) against the reference over ALL 512 desired masks, with the agent on its start cell and off
it, on dense grids (4x4: 7 free cells of 16; 5x5): tests/golden/sweep_imagine*_alias.npz, captured from the reference by tools/gen_golden.py (kind
'imagine_sweep').  Every op's return CRC, goal state (codes and agent, as arrays too), np_random position and key CRC, desired bits and home flag."""
import numpy as np
import pytest

import imagine_model as M

NAMES = M.sweep_fixture_names()


def _replay(name, wrong=False):
    meta, kw, d = M.load(name)
    env = M.ModelEnv(meta['env'], d['key0'], int(d['pos0']), wrong=wrong, **kw)
    rows, states = M.run_script(env, d['ops'], d['args'], lambda e, ret: e.last_state)
    return d, rows, states


def _bad(d, rows):
    return [i for i in range(len(rows)) if not np.array_equal(rows[i], d['rows'][i])]


def test_sweep_fixtures_present():
    assert {M.load(n)[1]['size'] for n in NAMES} == {(4, 4), (5, 5)}
    assert not set(NAMES) & set(M.fixture_names())             # (the op-script tests of the imagine_* fixtures do not pick these up)


@pytest.mark.parametrize('name', NAMES)
def test_fixture_holds_every_mask_on_both_sides_of_the_home_flag(name):
    meta, _, d = M.load(name)
    assert meta['kind'] == 'imagine_sweep' and meta['env'] == 'CraftingWorldEnvRay'
    ops, args = M.sweep_script(meta['steps'])
    assert np.array_equal(ops, d['ops']) and np.array_equal(args, d['args'])
    im = d['rows'][d['ops'] == M.I_IMAGINE]
    assert len(im) == 1024 and len(d['state_codes']) == 1024 and len(d['state_agent']) == 1024
    for home, part in ((1, im[:512]), (0, im[512:])):
        assert np.array_equal(part[:, M.COL_DESIRED], np.arange(512)) and (part[:, M.COL_HOME] == home).all()
    assert (im[:, M.COL_FLAGS] == (M.F_NEW | M.F_GOAL_KEPT | M.F_INIT_KEPT)).all()
    steps = d['rows'][d['ops'] == M.I_STEP]
    assert len(steps) == len(meta['steps']) and (steps[:, 1] == 0).all()     # (no step ended the episode)
    # the stream crosses a 624-word generation inside the sweep (the position falls), and the key changes with it
    assert (np.diff(im[:, M.COL_POS]) < 0).any() and len(set(im[:, M.COL_KEY].tolist())) > 1
    # nothing desired draws nothing: the stream stands where reset() left it, and where the last mask before the steps did (a step draws nothing)
    rows, first_off = d['rows'], int(np.flatnonzero(d['ops'] == M.I_STEP)[-1]) + 1
    assert d['args'][1] == 0 and np.array_equal(rows[1, M.COL_POS:M.COL_KEY + 1], rows[0, 1:3])
    assert d['args'][first_off] == 0 and np.array_equal(rows[first_off, M.COL_POS:M.COL_KEY + 1], rows[512, M.COL_POS:M.COL_KEY + 1])


@pytest.mark.parametrize('name', NAMES)
def test_model_replays_the_sweep(name):
    d, rows, states = _replay(name)
    for i in range(len(rows)):
        assert np.array_equal(rows[i], d['rows'][i]), 'op %d (%d, arg %d): model %s, reference %s' % (i, d['ops'][i], d['args'][i], rows[i], d['rows'][i])
    assert np.array_equal(np.array([c for c, _ in states], np.uint8), d['state_codes'])
    assert np.array_equal(np.array([a for _, a in states], np.uint8), d['state_agent'])


@pytest.mark.parametrize('name', NAMES)
def test_gotohouse_that_ignores_the_position_is_caught(name):
    """wrong only off the start cell: the first 512 masks replay, and the first miss is a GoToHouse mask with the same draws and another agent cell"""
    d, rows, _ = _replay(name, wrong='gotohouse')
    bad = _bad(d, rows)
    first_off = int(np.flatnonzero(d['ops'] == M.I_STEP)[-1]) + 1
    assert bad and bad[0] == first_off + (1 << M.T_GOTOHOUSE)
    i = bad[0]
    assert d['rows'][i, M.COL_HOME] == 0 and rows[i, M.COL_POS] == d['rows'][i, M.COL_POS] and rows[i, M.COL_AGENT] != d['rows'][i, M.COL_AGENT]
    assert all((d['rows'][j, M.COL_DESIRED] >> M.T_GOTOHOUSE) & 1 for j in bad)


@pytest.mark.parametrize('name', NAMES)
def test_movesticks_that_does_not_exclude_the_agents_cell_is_caught(name):
    """the draw range is one cell wider: the first miss is a MoveSticks mask among the first 512, on the start cell"""
    d, rows, _ = _replay(name, wrong='movesticks')
    bad = _bad(d, rows)
    assert bad
    i = bad[0]
    assert d['ops'][i] == M.I_IMAGINE and d['rows'][i, M.COL_HOME] == 1 and (d['rows'][i, M.COL_DESIRED] >> M.T_MOVESTICKS) & 1


@pytest.mark.parametrize('name', NAMES)
def test_movesticks_variant_misses_only_movesticks_masks(name):
    """After its first miss the wrong variant's stream has left the reference's, so every later row differs whatever its mask.  Here the wrong model runs
    op by op beside the right one and takes over its stream before every op: it then misses the reference at MoveSticks masks and nowhere else, on
    either side of the home flag, at most of them."""
    meta, kw, d = M.load(name)
    right = M.ModelEnv(meta['env'], d['key0'], int(d['pos0']), **kw)
    wrong = M.ModelEnv(meta['env'], d['key0'], int(d['pos0']), wrong='movesticks', **kw)
    bad = []
    for i in range(len(d['ops'])):
        wrong.np_random.set_state(right.np_random.get_state())
        wrong._push_rng()
        for env in (right, wrong):
            row, _ = M.run_script(env, d['ops'][i:i + 1], d['args'][i:i + 1], lambda e, ret: e.last_state)
            if env is right:
                assert np.array_equal(row[0], d['rows'][i]), i
            elif not np.array_equal(row[0], d['rows'][i]):
                bad.append(i)
    assert all(d['ops'][i] == M.I_IMAGINE and (d['rows'][i, M.COL_DESIRED] >> M.T_MOVESTICKS) & 1 for i in bad)
    home = d['rows'][bad, M.COL_HOME]
    assert (home == 1).sum() > 128 and (home == 0).sum() > 128      # (of 256 MoveSticks masks a side; a draw can fall on the same cell by chance)
