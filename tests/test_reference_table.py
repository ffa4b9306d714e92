"""GPU tier: the step rule of the HIP engine against what the REFERENCE classes answered on two whole transition tables -- tests/golden/table5_ray.npz (18 816
states on 5 x 5: every target / under / hold / side / init relation / achieved word, the agent at the centre and in a corner) and walls8_ray_alt.npz (1 296
states at every wall of 8 x 8, with the CRC of both reference classes' frame after every step).  The expectations are the recorded arrays: the oracle is never
called here, so a misreading of the reference that oracle and kernel share fails these tests and no other.  cw_expand, the step kernel itself, the frames of
both pixel engines in both rasters and cw_render_records.  Everything is bit-exact.  No timing."""
import numpy as np
import pytest
import torch

from golden_util import crc
from records_check import decode
from state_tables import DYNAMICS, load_table_fixture, same_table

pytestmark = pytest.mark.gpu

STYLES = [None, 'subset']                                   # the fixture's rule axis: equal, subset


@pytest.fixture(scope='module')
def table5():
    return load_table_fixture('table5_ray')


@pytest.fixture(scope='module')
def walls8():
    return load_table_fixture('walls8_ray_alt')


def _engine(fx, rule, step_num, **kw):
    """an engine of one env per state of the table, every state injected with set_state"""
    from gym_craftingworld_amd import CraftingWorldVecEnv
    env = CraftingWorldVecEnv(fx['n'], reward_style=STYLES[rule], auto_reset=False, seed=5, size=(fx['S'], fx['S']), max_steps=fx['max_steps'], **kw)
    env.reset()
    _inject(env, fx, step_num)
    return env


def _inject(env, fx, step_num):
    grid, init, agent, hold, ach = fx['table']
    env.set_state(grid=grid, init_grid=init, agent_rc=agent.astype(np.uint8), hold=hold.astype(np.uint8), achieved=ach.astype(np.uint16),
                  desired=fx['desired'].astype(np.uint16), step_num=np.full(fx['n'], step_num, np.int32))


def _want(fx, rule, step_num):
    """the fixture's columns of one reward rule and step_num, and `changed`: the successor differs from the state in grid, agent or hold"""
    grid, _, agent, hold, _ = fx['table']
    si = fx['step_nums'].index(step_num)
    want = {k: fx[k] for k in DYNAMICS + ('grid',)}
    want['reward'], want['done'] = fx['reward'][rule, si], fx['done'][rule, si]
    want['changed'] = ((fx['agent'] != agent[None]).any(axis=-1) | (fx['hold'] != hold[None]) | (fx['grid'] != grid[None]).any(axis=(-1, -2))).astype(np.int64)
    return want


def _own_new(sgrid, start, end):
    """the codes a successor grid [n, S, S] holds in the start cell and in the end cell"""
    j = np.arange(len(sgrid))
    return sgrid[j, start[:, 0], start[:, 1]].astype(np.int64), sgrid[j, end[:, 0], end[:, 1]].astype(np.int64)


def _stepped(env, fx, a):
    """one step(a) of every env -> the fixture's columns of that action, from get_state() and the step's outputs"""
    n = fx['n']
    _, rew, done, _ = env.step(torch.full((n,), a, dtype=torch.uint8, device='cuda'))
    rew, done = rew.cpu().numpy().astype(np.int64), done.cpu().numpy().astype(np.int64)
    st = env.get_state()
    assert np.array_equal(st['init_grid'], fx['table'][1]) and np.array_equal(st['desired'], fx['desired'])
    end = st['agent_rc'].astype(np.int64)
    own, new = _own_new(st['grid'], fx['table'][2], end)
    return dict(achieved=st['achieved'].astype(np.int64), agent=end, hold=st['hold'].astype(np.int64), own=own, new=new, grid=st['grid'], reward=rew, done=done,
                step_num=st['step_num'].astype(np.int64))


def _crcs(frames):
    f = frames.cpu().numpy()
    assert f.dtype == np.uint8
    return np.array([crc(x) for x in f.reshape((-1,) + f.shape[-3:])], np.int64).reshape(f.shape[:-3])


# ------------------------------------------------------------------------------------------------------------------------------ 1. cw_expand
@pytest.mark.parametrize('step_num', [3, 8])
@pytest.mark.parametrize('rule', [0, 1], ids=['equal', 'subset'])
def test_expand_on_the_whole_local_table(table5, rule, step_num):
    """18 816 envs, one state each: all six successors of every state -- grid, agent, hold, achieved, step_num + 1, reward, done and `changed` -- equal the
    reference's rows, under both reward rules, mid-episode and one step before the time-out"""
    fx = table5
    n, S = fx['n'], fx['S']
    env = _engine(fx, rule, step_num, obs_mode='state')
    r = env.expand()
    assert tuple(r['hdr'].shape) == (6, n, 16)
    d = decode(r['hdr'].cpu().numpy(), r['slot_pos'].cpu().numpy(), S)
    d = {k: v.reshape((6, n) + v.shape[1:]) for k, v in d.items()}
    start = fx['table'][2]
    pairs = [_own_new(d['grid'][a], start, d['agent'][a]) for a in range(6)]
    got = dict(achieved=d['achieved'], agent=d['agent'], hold=d['hold'], grid=d['grid'], own=np.stack([p[0] for p in pairs]), new=np.stack([p[1] for p in pairs]),
               reward=r['reward'].cpu().numpy().astype(np.int64), done=r['done'].cpu().numpy().astype(np.int64), changed=r['changed'].cpu().numpy().astype(np.int64))
    want = _want(fx, rule, step_num)
    same_table(want, got, fx['cases'], tag='expand(), rule %d, step_num %d: ' % (rule, step_num))
    assert np.array_equal(r['achieved_mask'].cpu().numpy().view(np.uint16).astype(np.int64), fx['achieved'])
    assert (d['step_num'] == step_num + 1).all() and (d['desired'] == fx['desired'][None]).all() and np.array_equal(d['held_code'], fx['hold'])
    # the flag word: bit 0 (no step yet) cleared, bit 1 the reward rule, the success count in bits 2-15 one up where the step paid max_steps
    assert np.array_equal(d['flags'], 2 * rule + 4 * (want['reward'] == fx['max_steps']))
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 2. the step kernel itself
@pytest.mark.parametrize('rule', [0, 1], ids=['equal', 'subset'])
def test_the_step_kernel_on_the_whole_local_table(table5, rule):
    """the same table through set_state + one step() of each action for every env, one step before the time-out: get_state()'s fields, reward and done"""
    fx = table5
    step_num = fx['max_steps'] - 1
    env = _engine(fx, rule, step_num, obs_mode='state')
    want = _want(fx, rule, step_num)
    for a in range(6):
        if a:
            _inject(env, fx, step_num)
        got = _stepped(env, fx, a)
        assert (got.pop('step_num') == step_num + 1).all(), a
        same_table({k: want[k][a] for k in got}, got, fx['cases'], tag='step(%d), rule %d: ' % (a, rule))
        assert got['done'].all()                                  # (every env has timed out; without auto-reset it stays in its last state)
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 3. frames
@pytest.mark.parametrize('raster', ['ray', 'alt'])
@pytest.mark.parametrize('obs_mode', ['pixels', 'pixels_dirty'])
def test_the_frames_of_the_pixel_engines_on_the_wall_table(walls8, obs_mode, raster):
    """1 296 states at every wall of 8 x 8 on the full-frame and on the dirty-cell engine, both rasters: after set_state and one step of each action the
    observation has the CRC of the reference class's obs_image.astype(uint8) -- CraftingWorldEnvRay's for raster 'ray', CraftingWorldEnvAltObs's (values above
    255 modulo 256) for 'alt' -- and the state, reward and done are the reference's.  The ray engines run the equal rule, the alt engines the subset rule."""
    fx = walls8
    rule = int(raster == 'alt')
    env = _engine(fx, rule, 3, obs_mode=obs_mode, raster=raster)
    want = _want(fx, rule, 3)
    want['frame'] = fx['crc_' + raster]
    for a in range(6):
        if a:
            _inject(env, fx, 3)
        got = _stepped(env, fx, a)
        assert (got.pop('step_num') == 4).all(), a
        got['frame'] = _crcs(env._observation()['observation'])
        same_table({k: want[k][a] for k in got}, got, fx['cases'], tag='%s / %s, step(%d): ' % (obs_mode, raster, a))
    env.close()


@pytest.mark.parametrize('raster', ['ray', 'alt'])
def test_render_records_of_the_wall_tables_successors(walls8, raster):
    """cw_render_records of expand()'s 6 x 1 296 rows: the frame of every successor has the reference class's CRC"""
    fx = walls8
    env = _engine(fx, 0, 3, obs_mode='state', raster=raster)
    r = env.expand()
    d = decode(r['hdr'].cpu().numpy(), r['slot_pos'].cpu().numpy(), fx['S'])
    got = dict(grid=d['grid'].reshape(fx['grid'].shape), agent=d['agent'].reshape(6, fx['n'], 2), hold=d['hold'].reshape(6, fx['n']),
               achieved=d['achieved'].reshape(6, fx['n']))
    same_table({k: fx[k] for k in got}, got, fx['cases'], tag='expand() on the wall table: ')
    frames = env.render_records(r['hdr'], r['slot_pos'])
    assert tuple(frames.shape) == (6, fx['n']) + tuple(env.frame_shape) and frames.dtype == torch.uint8
    same_table({'frame': fx['crc_' + raster]}, {'frame': _crcs(frames)}, fx['cases'], tag='render_records(), %s: ' % raster)
    env.close()
