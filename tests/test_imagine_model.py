"""The numpy model of imagine_obs() / sample_state() / generate_fixed_initial_state() (tests/imagine_model.py) replays every fixture captured from the
reference (tests/golden/imagine_*.npz, tools/gen_golden.py kind 'imagine') exactly -- which is what licenses it as the comparator of the GPU tests
(tests/test_imagine.py) and as the fake engine's two entry points (tests/fake_engine_imagine.py)."""
import numpy as np
import pytest

import imagine_model as M

NAMES = M.fixture_names()


def test_fixtures_present():
    kinds = {M.load(n)[0]['env'] for n in NAMES}
    assert kinds == {'CraftingWorldEnvRay', 'CraftingWorldEnvAltObs', 'CraftingWorldEnvOneHot', 'CraftingWorldEnvFlat'}
    sizes = {M.load(n)[1]['size'][0] for n in NAMES if M.load(n)[0]['env'] == 'CraftingWorldEnvRay'}
    assert {5, 6, 8, 21} <= sizes


def _replay(name, wrong=False):
    meta, kw, d = M.load(name)
    env = M.ModelEnv(meta['env'], d['key0'], int(d['pos0']), wrong=wrong, **kw)
    rows, states = M.run_script(env, d['ops'], d['args'], lambda e, ret: e.last_state)
    return meta, d, rows, states


@pytest.mark.parametrize('name', NAMES)
def test_model_replays_the_reference(name):
    meta, d, rows, states = _replay(name)
    ops = d['ops']
    for i in range(len(ops)):
        assert np.array_equal(rows[i], d['rows'][i]), 'op %d (%d, arg %d): model %s, reference %s' % (i, ops[i], d['args'][i], rows[i], d['rows'][i])
    if 'state_codes' in d:
        assert np.array_equal(np.array([c for c, _ in states], np.uint8), d['state_codes'])
        assert np.array_equal(np.array([a for _, a in states], np.uint8), d['state_agent'])


@pytest.mark.parametrize('name', NAMES)
def test_fixture_meets_its_conditions(name):
    """what tools/gen_golden.py asserted when it chose the script: every task bit imagined, GoToHouse off the start cell and back on it, two houses,
    nothing desired, every call returning a new image and leaving desired_goal / INIT_OBS_VECTOR alone"""
    _, _, d = M.load(name)
    im = d['rows'][d['ops'] == M.I_IMAGINE]
    want = lambda t: (im[:, M.COL_DESIRED] >> t) & 1  # noqa: E731
    assert all(want(t).any() for t in range(9))
    goto = want(M.T_GOTOHOUSE) == 1
    off = np.flatnonzero(goto & (im[:, M.COL_HOME] == 0))
    assert len(off) and (goto & (im[:, M.COL_HOME] == 1))[off[0]:].any()
    assert (goto & (want(M.T_BUILDHOUSE) == 1)).any() and (im[:, M.COL_DESIRED] == 0).any()
    assert (im[:, M.COL_FLAGS] == (M.F_NEW | M.F_GOAL_KEPT | M.F_INIT_KEPT)).all()
    assert (im[:, M.COL_DTYPE] == 8 * 4).all()                 # int64
    # nothing desired: no draw (the stream stands where the op before left it)
    zero = np.flatnonzero((d['ops'] == M.I_IMAGINE) & (d['args'] == 0))
    assert len(zero) and all(np.array_equal(d['rows'][i, M.COL_POS:M.COL_KEY + 1], d['rows'][i - 1, M.COL_POS:M.COL_KEY + 1]) for i in zero)


def test_a_wrong_model_is_caught():
    """a model that moves the agent to the house wherever it stands (the start cell's agent instead of the current cell's, ray.py:274-276) fails every fixture"""
    for name in NAMES:
        meta, d, rows, _ = _replay(name, wrong=True)
        bad = [i for i in range(len(rows)) if not np.array_equal(rows[i], d['rows'][i])]
        assert bad, name
        i = bad[0]
        assert d['ops'][i] == M.I_IMAGINE and d['rows'][i, M.COL_HOME] == 0 and (d['rows'][i, M.COL_DESIRED] >> M.T_GOTOHOUSE) & 1
        assert rows[i, M.COL_POS] == d['rows'][i, M.COL_POS]      # (same draws: only the agent's cell is wrong)


def test_sample_state_matches_numpy_indexing():
    for seed in range(20):
        S = 4 + seed % 5
        cells = M.sample_state(S, np.random.RandomState(seed))
        rs = np.random.RandomState(seed)
        state = np.zeros((S * S, 1, 12), dtype=int)
        state[:12, 0, :] = np.diag([1] * 9 + [0] * 3)
        perm = np.arange(S * S)
        rs.shuffle(perm)
        state = state[perm].reshape(S, -1, 12)
        codes, agent = M.codes_of_cells(S, cells)
        assert np.array_equal(M.one_hot(codes, agent), state)
