"""CPU tier: the hand-built states of the expand and snapshot tests (tests/state_tables.py).  What the wall tables exercise is counted here from the
oracle's successors alone -- the GPU tests that use them compare, these say what is compared -- and every painted state is one the oracle takes and the
packed record format holds.  No GPU."""
import numpy as np
import pytest

from expand_check import oracle_successors
from records_check import POS_HELD, decode, encode
from state_tables import (LARGE_CAP, oracle_frame, painted_batch, painted_states, table_coverage, table_desired, wall_table)

MAX_STEPS = 9
ANCHORS_8 = [(0, 0), (0, 7), (7, 0), (7, 7), (0, 4), (4, 7), (7, 4), (4, 0)]


def far_corners(S):
    return [(S - 1, S - 1), (0, S - 1), (S - 1, 0)]


def _dense(table, desired=1):
    grid, init, agent, hold, ach = table
    z = np.zeros(len(hold), np.int64)
    return dict(grid=grid, agent=agent, hold=hold, achieved=ach, desired=z + desired, step_num=z + 3, flags=z)


def test_the_full_span_is_the_table_of_test_expand():
    """wall_table(span='full') has _table()'s cases at an anchor, in its order: the same under / target / hold / achieved words, the target on the same side,
    the same object of the init grid moved onto it"""
    grid, init, agent, hold, ach = wall_table(8, [(2, 2)], 9408, span='full')
    assert len(hold) == 9408 and (agent == 2).all()
    from itertools import product
    ref = [c for c in product(range(9), (0, 1, 2, 3, 7, 8), range(4), range(4), range(4), range(3)) if not (c[0] and c[0] == c[1])]
    dr = [(-1, 0), (0, 1), (1, 0), (0, -1)]
    for j in (0, 1, 77, 4000, 9407):
        tgt, under, h, side, initv, achv = ref[j]
        tr, tc = 2 + dr[side][0], 2 + dr[side][1]
        assert (grid[j, 2, 2], grid[j, tr, tc], hold[j], ach[j]) == (under, tgt, h, (0, 8, 0x1FF)[achv]) and (grid[j] != 0).sum() == (under != 0) + (tgt != 0)
        moved = {0: 0, 1: 1, 2: 2 if h != 3 else 3, 3: 5}[initv]
        assert init[j, tr, tc] == moved and sorted(init[j][init[j] != 0].tolist()) == list(range(1, 9))


def test_parking_is_clear_of_the_agent_and_the_sizes_are_capped():
    for S, anchors in ((8, ANCHORS_8 + [(3, 3), (4, 4)]), (182, far_corners(182))):
        grid, init, agent, hold, ach = wall_table(S, anchors, 10 ** 6)
        assert len(hold) == 144 * len(anchors)
        for j in range(len(hold)):
            ar, ac = agent[j]
            r, c = np.nonzero(init[j])
            far = np.abs(r - ar) >= 2                                             # (every parked object; the one moved onto the target is the exception)
            assert far.sum() >= 7 and (np.abs(r[~far] - ar) + np.abs(c[~far] - ac) <= 1).all()
    with pytest.raises(ValueError):
        wall_table(8, ANCHORS_8, 144 * 8 - 1)
    with pytest.raises(ValueError):
        wall_table(182, far_corners(182) + [(0, 0)], 10 ** 6)                      # 576 states: above the cap of the large sizes, whatever the caller allows
    assert LARGE_CAP == 512
    for bad in (dict(S=7, anchors=[(0, 0)]), dict(S=8, anchors=[(8, 0)]), dict(S=8, anchors=[]), dict(S=8, anchors=[(0, 0)], span='whole')):
        with pytest.raises(ValueError):
            wall_table(max_states=10 ** 6, **bad)


def test_the_eight_wall_table_covers_what_the_interior_table_does():
    """case (a): 8 x 8, the four corners and the four mid-edge cells, the full span: 75 264 states; the floors of test_the_whole_local_transition_table"""
    table = wall_table(8, ANCHORS_8, 75264, span='full')
    assert len(table[3]) == 75264
    okw = dict(size=(8, 8), max_steps=MAX_STEPS)
    states = _dense(table)
    states['desired'] = table_desired(table, okw)
    cov = table_coverage(states, oracle_successors(states, table[1], okw))
    print(cov)
    assert min(cov['gains']) >= 100 and min(cov['losses']) >= 400 and cov['changed'] >= 50000 and cov['unchanged'] >= 50000
    assert min(cov['blocked_moves']) >= 10000                                      # every move runs into its wall


@pytest.mark.parametrize('S', [182, 255])
def test_the_far_corner_table_covers_the_large_grids(S):
    """case (b): the three far corners, the reduced span: 432 states whose cells, rows and columns need all 16 / 8 bits"""
    table = wall_table(S, far_corners(S), 512)
    okw = dict(size=(S, S), max_steps=MAX_STEPS)
    states = _dense(table)
    assert len(states['hold']) == 432
    suc = oracle_successors(states, table[1], okw)
    cov = table_coverage(states, suc)
    _, pos = encode(states)
    above = int(((pos > 32767) & (pos < POS_HELD)).sum())
    print(S, cov, 'slot cells above 32 767:', above)
    assert min(cov['gains']) >= 2 and min(cov['losses']) >= 10 and min(cov['blocked_moves']) >= 100 and cov['pickups'] >= 40 and cov['drops'] >= 40
    assert above >= 300 and (states['agent'].max(axis=1) >= 128).all()
    assert (suc['agent'].max(axis=-1) >= 128).all()                                # ... and so does every successor's


@pytest.mark.parametrize('S', [5, 8, 21, 255])
def test_painted_states_are_states_of_the_oracle_and_of_the_record_format(S):
    """case (c): OracleEnv.set_state takes every entry and gives it back with the frame oracle_frame paints; no entry has more than eight objects or an init
    grid with an object twice (what cw_set_state refuses); encode / decode round-trip it -- at 255 with most cells above 32 767"""
    from oracle import OracleEnv
    ps = painted_states(S)
    names = [p[0] for p in ps]
    assert len(ps) == 22 and len(set(names)) == 22
    assert sorted({p[4] for p in ps if 'empty cell' in p[0]}) == [0, 1, 2, 3] and sorted({p[4] for p in ps if 'standing on' in p[0]}) == [0, 1, 2, 3]
    corners = {(p[3], p[4] != 0) for p in ps if p[0].startswith('corner')}
    assert corners == {((r, c), h) for r in (0, S - 1) for c in (0, S - 1) for h in (False, True)}
    by = dict(zip(names, ps))
    assert by['an object in cell 0'][1][0, 0] and by['an object in cell S*S - 1'][1][S - 1, S - 1] and by['an object in cell 0'][2][0, 0]
    assert sorted(by['rock and bread both gone'][1][by['rock and bread both gone'][1] != 0].tolist()) == [1, 2, 3, 5, 7, 8]
    assert by['a house under the agent'][1][by['a house under the agent'][3]] == 7
    envs = {alt: OracleEnv(size=(S, S), max_steps=MAX_STEPS, alt_obs=alt) for alt in (False, True)}
    for name, grid, init, agent, hold in ps:
        assert (grid != 0).sum() + (hold != 0) <= 8 and grid.max() <= 8 and all((init == k).sum() == 1 for k in range(1, 9)), name
        assert not hold or grid[agent] not in (4, 5), name                         # (nobody stands on a rock or a tree)
        for alt, o in envs.items():
            o.set_state(grid, init, agent, hold, 0, 1, 3)
            st = o.state()
            assert np.array_equal(st['grid'], grid) and np.array_equal(st['init_grid'], init) and (st['agent'], st['hold']) == (agent, hold), name
            assert np.array_equal(st['obs'], oracle_frame(grid, agent, hold, alt)), name
    _, grid, init, agent, hold = painted_batch(S, 48)
    assert np.array_equal(grid[22:44], grid[:22]) and np.array_equal(agent[44:], agent[:4])
    dense = dict(grid=grid, agent=agent.astype(np.int64), hold=hold.astype(np.int64), achieved=np.arange(48), desired=np.arange(48) + 1,
                 step_num=np.full(48, 3), flags=np.zeros(48, np.int64))
    hdr, pos = encode(dense)
    back = decode(hdr, pos.view(np.int16), S)                                      # (as the engine's int16 tensors hand them over)
    for k in ('grid', 'agent', 'hold', 'achieved', 'desired', 'step_num', 'flags'):
        assert np.array_equal(back[k], dense[k]), k
    assert np.array_equal(back['held_code'], dense['hold'])
    if S == 255:
        assert int(((pos > 32767) & (pos < POS_HELD)).sum()) >= 100 and agent.max() == 254


def test_sticks_over_sticks_doubles_the_alt_pixel():
    """the one reachable pixel whose reference value leaves a byte: sticks held over a sticks cell, (90, 164, 320) -> (90, 164, 64) in the uint8 frame"""
    S = 8
    name, grid, init, agent, hold = [p for p in painted_states(S) if p[0] == 'sticks held over a sticks cell'][0]
    assert hold == 1 and grid[agent] == 1
    img = oracle_frame(grid, agent, hold, True)
    assert img.shape == (27, 24, 3) and img[3 * agent[0], 3 * agent[1]].tolist() == [90, 164, 320 % 256]
    assert oracle_frame(grid, agent, 0, True)[3 * agent[0], 3 * agent[1]].tolist() == [45, 82, 160]
    assert oracle_frame(grid, agent, hold, False).shape == (32, 32, 3)
