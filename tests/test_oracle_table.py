"""CPU tier: the C oracle against what the REFERENCE classes answered on the two table fixtures (tests/golden/table5_ray.npz, walls8_ray_alt.npz).  Every GPU
expectation of this suite comes from the oracle; the trajectory fixtures tie it to the reference on the states a trajectory visits, these tie it on whole
transition tables: every (target, under, hold, side, init relation, achieved word, wall) class under both reward rules, mid-episode and one step before the
time-out, and both rasterisers on every successor of the wall table.  Field for field, row for row.  No GPU."""
import numpy as np
import pytest

from expand_check import oracle_successors
from golden_util import crc
from state_tables import DYNAMICS, TABLE_FIXTURES, load_table_fixture, oracle_frame, same_table


@pytest.fixture(scope='module')
def fixtures():
    return {name: load_table_fixture(name) for name in TABLE_FIXTURES}


def _oracle_rows(fx, rule, step_num):
    """oracle_successors of the fixture's table under reward rule `rule` (0 equal, 1 subset) at step_num -> the fixture's columns"""
    grid, init, agent, hold, ach = fx['table']
    n = fx['n']
    z = np.zeros(n, np.int64)
    states = dict(grid=grid, agent=agent, hold=hold, achieved=ach, desired=fx['desired'], step_num=z + step_num, flags=z + 2 * rule)
    suc = oracle_successors(states, init, dict(size=(fx['S'], fx['S']), max_steps=fx['max_steps']))
    j = np.arange(n)
    end = suc['agent']
    got = dict(achieved=suc['achieved'], agent=suc['agent'], hold=suc['hold'], grid=suc['grid'], reward=suc['reward'], done=suc['done'].astype(np.int64),
               own=np.stack([suc['grid'][a][j, agent[:, 0], agent[:, 1]] for a in range(6)]).astype(np.int64),
               new=np.stack([suc['grid'][a][j, end[a, :, 0], end[a, :, 1]] for a in range(6)]).astype(np.int64))
    assert (suc['step_num'] == step_num + 1).all() and (suc['desired'] == fx['desired'][None]).all()
    return got, suc


@pytest.mark.parametrize('rule', [0, 1], ids=['equal', 'subset'])
@pytest.mark.parametrize('name,step_num', [(n, s) for n, spec in TABLE_FIXTURES.items() for s in spec['step_nums']])
def test_the_oracle_answers_what_the_reference_answered(fixtures, name, rule, step_num):
    fx = fixtures[name]
    got, _ = _oracle_rows(fx, rule, step_num)
    si = fx['step_nums'].index(step_num)
    want = {k: fx[k] for k in DYNAMICS + ('grid',)}
    want['reward'], want['done'] = fx['reward'][rule, si], fx['done'][rule, si]
    same_table(want, got, fx['cases'], tag='%s, rule %d, step_num %d: the oracle\'s ' % (name, rule, step_num))


def test_the_oracles_rasterisers_paint_what_the_reference_classes_painted(fixtures):
    """oracle_frame of every successor of the wall table, ray and alt, has the CRC of the reference class's obs_image.astype(uint8) after that step"""
    fx = fixtures['walls8_ray_alt']
    n = fx['n']
    suc = fx                                                              # (the reference's own successors: the rasterisers alone are under test)
    for alt, column in ((False, 'crc_ray'), (True, 'crc_alt')):
        seen = {}
        got = np.zeros((6, n), np.int64)
        for a in range(6):
            for j in range(n):
                key = (suc['grid'][a, j].tobytes(), tuple(suc['agent'][a, j].tolist()), int(suc['hold'][a, j]))
                if key not in seen:
                    seen[key] = crc(oracle_frame(suc['grid'][a, j], suc['agent'][a, j], suc['hold'][a, j], alt))
                got[a, j] = seen[key]
        assert len(seen) >= n
        same_table({column: fx[column]}, {column: got}, fx['cases'], tag='the oracle\'s frame: ')
