"""GPU tier of the exact search: CraftingWorldVecEnv.reach -- expand() + seen_insert() + torch compaction -- against seen_check.reference_reach (breadth-first
over the CPU oracle, pinned to brute force by tests/test_seen_logic.py), against plan() where plan() reaches, and against itself.  The plans it returns go
back through simulate().  Everything is exact.  No timing."""
import numpy as np
import pytest
import torch

from engines import ENGINES, K5, N1
from masked_check import spread
from oracle_replay import make_env, np_states
from records_check import decode
from records_gpu import dev as _dev, walk_goals
from seen_check import REACH_MAX_STEPS, REACH_N, REACH_SEEDS, reach_reference, reference_reach, seed_states

pytestmark = pytest.mark.gpu

DEPTH = 10


def _start_engine(size):
    """the REACH_N envs of seen_check.oracle_starts on the card, as reset() leaves them"""
    env, _, _ = make_env(REACH_N, *seed_states(REACH_SEEDS[size]), obs_mode='state', auto_reset=False, size=(size, size), max_steps=REACH_MAX_STEPS)
    env.reset()
    return env


def _plans_hold(env, r, hdr=None, slot_pos=None, env_of=None):
    """the plans of reach() through simulate(): a solved row ends done, by success, at length == distance; an unsolved row's plan is zeros"""
    dist, plan = r['distance'].cpu().numpy(), r['plan']
    D = plan.shape[0]
    assert plan.dtype == torch.uint8 and r['distance'].dtype == torch.int32 and tuple(plan.shape) == (D, len(dist))
    assert torch.equal(r['first_action'], plan[0])
    solved = dist > 0
    assert ((dist == -1) | solved).all() and (dist <= D).all()
    p = plan.cpu().numpy()
    assert (p[:, ~solved] == 0).all() and (p <= 5).all()
    assert (p[np.arange(D)[:, None] >= np.where(solved, dist, 0)[None, :]] == 0).all()          # zeros behind a plan's end
    if hdr is None:
        s = env.simulate(plan)
    else:
        s = env.simulate(plan, hdr, slot_pos, env_of)
    ret, length, done = s['ret'].cpu().numpy(), s['length'].cpu().numpy(), s['done'].cpu().numpy()
    assert done[solved].all() and np.array_equal(length[solved], dist[solved])
    assert np.array_equal(ret[solved], env.MAX_STEPS - (dist[solved] - 1))
    return dist


@pytest.mark.parametrize('size', [5, 8])
def test_reach_against_the_reference(size):
    """12 start rows, depth 10: the distances are the oracle's breadth-first ones (5 x 5: 6 rows solved, in 2 .. 10 steps; 8 x 8: 5 rows, in 3 .. 9), the
    plans succeed at exactly that length, and two calls agree"""
    dense, _, ref = reach_reference(size, DEPTH)
    env = _start_engine(size)
    got = decode(env.hdr.cpu().numpy(), env.slot_pos.cpu().numpy(), size)
    for k in ('grid', 'agent', 'hold', 'achieved', 'desired', 'step_num', 'flags'):
        assert np.array_equal(got[k], dense[k]), k                                   # the engine starts where the oracle starts
    r = env.reach(DEPTH, max_rows=1 << 16)
    dist = _plans_hold(env, r)
    assert np.array_equal(dist, ref['distance']), (dist, ref['distance'])
    assert (dist > 0).sum() * 4 >= REACH_N and (dist < 0).any() and dist.max() >= 9
    assert r['searched_depth'] == DEPTH == ref['searched_depth'] and len(r['frontier']) == DEPTH and r['frontier'][:3] == ref['frontier'][:3]
    assert r['states'] == env.seen_size >= ref['states'] and (env.seen_overflow, env.seen_collisions) == (0, 0)   # (the reference merges slot orders too)
    again = env.reach(DEPTH, max_rows=1 << 16)
    assert torch.equal(again['distance'], r['distance']) and torch.equal(again['plan'], r['plan']) and again['states'] == r['states']
    env.close()


def test_max_rows_stops_the_search_at_level_3():
    """5 x 5: the frontiers hold 35, 55 and 69 states after levels 1, 2 and 3 (the oracle's count); max_rows = 60 stops before the fourth expansion"""
    _, _, ref = reach_reference(5, DEPTH)
    assert ref['frontier'][:4] == [12, 35, 55, 69]
    env = _start_engine(5)
    env.seen_reserve(1 << 12)                                                        # a set of the caller's is used as it is, and cleared
    env.seen_insert(env.hdr, env.slot_pos)
    r = env.reach(DEPTH, max_rows=60)
    dist = _plans_hold(env, r)
    assert r['searched_depth'] == 3 and env.seen_slots == 1 << 13
    want = np.where((ref['distance'] > 0) & (ref['distance'] <= 3), ref['distance'], -1)
    assert np.array_equal(dist, want) and sorted(dist[dist > 0].tolist()) == [2, 3]
    env.close()


@pytest.mark.parametrize('engine', list(ENGINES))
def test_reach_against_plan_on_every_engine(engine):
    """70 envs, depth 5: distance == d exactly where plan()'s best return is that of a success at step d"""
    env, _, _ = make_env(N1, *np_states(N1, 96000), **ENGINES[engine], **K5)
    env.reset()
    spread(env, 4, 8)
    walk_goals(env, 3, 96500)
    want = env.plan(5, fields=('best_q',))['best_q'].cpu().numpy()
    r = env.reach(5, max_rows=1 << 14)
    dist = _plans_hold(env, r)
    assert np.array_equal(dist > 0, want > 0)
    assert np.array_equal(env.MAX_STEPS - (dist[dist > 0] - 1), want[dist > 0])
    assert (dist > 0).sum() >= 5 and (dist < 0).sum() >= 5 and len(set(dist[dist > 0].tolist())) >= 2, dist
    env.close()


def test_start_rows_of_the_caller():
    """two rows of one env that differ only in step_num, 2 and 12 of max_steps 17, depth 8: the time-out cuts the second row's search after five steps and
    not the first's -- three envs whose goals are 6, 7 and 8 steps away lose their second row, three with goals 3, 5 and 2 steps away keep it; a row whose
    env_of entry is negative takes no part"""
    seeds = (4017, 4031, 4013, 4029, 4004, 4117)
    env, _, _ = make_env(len(seeds), *seed_states(seeds), obs_mode='state', auto_reset=False, **K5)
    env.reset()
    envs = np.array([0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 0], np.int64)
    hdr, pos = env.hdr.cpu().numpy()[envs], env.slot_pos.cpu().numpy()[envs]
    hdr[:, 8], hdr[:, 9] = np.where(np.arange(13) % 2 == 0, 2, 12), 0
    eo = envs.copy()
    eo[12] = -3
    r = env.reach(8, _dev(hdr), _dev(pos, np.int16), _dev(eo, np.int32), max_rows=1 << 16)
    dist = _plans_hold(env, r, _dev(hdr), _dev(pos, np.int16), _dev(envs, np.int32))
    assert dist.tolist() == [6, -1, 7, -1, 8, -1, 3, 3, 5, 5, 2, 2, -1]
    dense = decode(hdr, pos, 5)
    ref = reference_reach({k: dense[k] for k in ('grid', 'agent', 'hold', 'achieved', 'desired', 'step_num', 'flags')}, env.get_state()['init_grid'][envs], 8,
                          dict(size=(5, 5), max_steps=K5['max_steps']))
    assert np.array_equal(np.where(eo < 0, -1, ref['distance']), dist)
    assert r['searched_depth'] == 8
    env.close()
