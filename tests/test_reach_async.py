"""GPU tier of the search without a host round trip: CraftingWorldVecEnv.reach_async (cw_reach: the cw_reach_*_kernel family and the visited set's own
kernels) against VecEnv.reach() on the same start rows with the same max_rows -- every output byte for byte, the choice among equally short plans included
(reach_check.check_reach_call, itself tested on the CPU by tests/test_reach_async_logic.py) --, against seen_check.reach_reference and plan(), and the plans
through simulate().  Every comparison is exact.  No timing."""
import ctypes as C

import numpy as np
import pytest
import torch

from engines import ENGINES, K5, N1, n_cu
from masked_check import spread, take
from oracle_replay import make_env, np_states
from reach_check import check_reach_call, rows_of
from records_gpu import REACH_OUT as OUT, SENT, dev as _dev, reach_sentinel_out as _sentinel_out, tiled_rows as _tiled, walk_goals
from seen_check import REACH_MAX_STEPS, REACH_N, REACH_SEEDS, reach_reference, seed_states

pytestmark = pytest.mark.gpu

DEPTH = 10


def _start_engine(size):
    """the REACH_N envs of seen_check.oracle_starts on the card, as reset() leaves them (tests/test_reach.py's engines)"""
    env, _, _ = make_env(REACH_N, *seed_states(REACH_SEEDS[size]), obs_mode='state', auto_reset=False, size=(size, size), max_steps=REACH_MAX_STEPS)
    env.reset()
    return env


def _host(r):
    return {f: t.cpu().numpy() for f, t in r.items()}


def _clean(env):
    assert (env.seen_overflow, env.seen_collisions) == (0, 0)


def _both(env, depth, hdr=None, pos=None, eo=None, *, max_rows, engine=False):
    """reach() and then reach_async() into sentinel-filled buffers from the same start rows with the same max_rows: every output equal, the set clean after
    both, the engine (engine=True) byte for byte as before the call -> (reach()'s result, reach_async()'s as numpy)"""
    ref = env.reach(depth, hdr, pos, eo, max_rows=max_rows)
    _clean(env)
    m0 = len(ref['distance'])
    out = _sentinel_out(depth, m0)
    before = take(env) if engine else None
    r = env.reach_async(depth, hdr, pos, eo, max_rows=max_rows, out=out)
    assert all(r[f] is out[f] for f, _ in OUT) and r['states'].dtype == torch.int64 and tuple(r['states'].shape) == (1,)
    torch.cuda.synchronize()
    got = _host(r)
    check_reach_call(ref, got, SENT, before, take(env) if engine else None)
    _clean(env)
    assert int(got['states'][0]) == env.seen_size
    return ref, got


def _plans_hold(env, got, hdr=None, pos=None, eo=None):
    """the plans through simulate() (the shape of tests/test_reach.py's check): a solved row ends done, by success, at length == distance"""
    dist = got['distance']
    solved = dist > 0
    plan = _dev(got['plan'])
    s = env.simulate(plan) if hdr is None else env.simulate(plan, hdr, pos, eo)
    ret, length, done = s['ret'].cpu().numpy(), s['length'].cpu().numpy(), s['done'].cpu().numpy()
    assert done[solved].all() and np.array_equal(length[solved], dist[solved])
    assert np.array_equal(ret[solved], env.MAX_STEPS - (dist[solved] - 1))
    return dist


# ------------------------------------------------------------------------------------------------------------------------------ 1. against reach()
@pytest.mark.parametrize('size', [5, 8])
def test_against_reach_and_the_reference(size):
    """12 start rows, depth 10, the engine's own records: every output is reach()'s, the distances are the oracle's breadth-first ones, the plans succeed at
    exactly that length"""
    _, _, ref = reach_reference(size, DEPTH)
    env = _start_engine(size)
    env.seen_reserve(1 << 16)
    r, got = _both(env, DEPTH, max_rows=1 << 14, engine=True)
    dist = _plans_hold(env, got)
    assert np.array_equal(dist, ref['distance']) and got['searched_depth'][0] == DEPTH and got['frontier'][:3].tolist() == ref['frontier'][:3]
    assert (got['frontier'] > 0).all() and env.reach_bytes > 0
    env.close()


@pytest.mark.parametrize('engine', list(ENGINES))
def test_on_every_engine_against_reach_and_plan(engine):
    """70 envs, depth 5: reach()'s outputs, distance == d exactly where plan()'s best return is that of a success at step d, and the engine -- states,
    streams, buffers, frames, counters -- byte for byte unchanged"""
    env, _, _ = make_env(N1, *np_states(N1, 96000), **ENGINES[engine], **K5)
    env.reset()
    spread(env, 4, 8)
    walk_goals(env, 3, 96500)
    want = env.plan(5, fields=('best_q',))['best_q'].cpu().numpy()
    env.seen_reserve(1 << 16)
    _, got = _both(env, 5, max_rows=1 << 14, engine=True)
    dist = _plans_hold(env, got)
    assert np.array_equal(dist > 0, want > 0) and np.array_equal(env.MAX_STEPS - (dist[dist > 0] - 1), want[dist > 0])
    assert (dist > 0).sum() >= 5 and (dist < 0).sum() >= 5
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 2. shapes
@pytest.fixture(scope='module')
def engine5():
    env = _start_engine(5)
    env.seen_reserve(1 << 20)
    yield env
    env.close()


@pytest.mark.parametrize('M0', [0, 1, 63, 64, 65, 257])
def test_start_row_counts(engine5, M0):
    """M0 start rows tiled from the 12 envs, depth 5: frontiers on both sides of a wave, of a workgroup and (257 rows: 6 * 1 216 rows at level 2) of a chunk"""
    env = engine5
    hdr, pos, eo = _tiled(env, M0)
    ref, got = _both(env, 5, hdr, pos, eo, max_rows=1 << 13, engine=M0 == 65)
    if M0:
        assert np.array_equal(got['distance'][:min(M0, REACH_N)], env.reach(5, max_rows=1 << 13)['distance'].cpu().numpy()[:M0])
        assert got['frontier'][0] == M0
    else:
        assert got['frontier'].tolist() == [0] * 5 and got['searched_depth'][0] == 5 and int(got['states'][0]) == 0
    if M0 == 257:
        assert rows_of(int(got['frontier'][1])) > 4096 and rows_of(int(got['frontier'][0])) < 4096


def test_past_the_first_grid_stride_round(engine5):
    """enough tiled start rows that the 6 F rows of level 4 pass the lanes the row kernels are launched with (8 workgroups of 256 per CU): at 5 x 5 twelve
    start rows grow to 69 states at level 3"""
    from gym_craftingworld_amd import _lib as L
    env = engine5
    max_rows = 1 << 17
    lanes = 256 * L.load().cwh_reach_grid_of(rows_of(max_rows), n_cu())
    assert lanes == 256 * 8 * n_cu()                                              # (the cap, not the rows, decides the grid)
    M0 = 12 * (lanes // (6 * 69) + 2)
    hdr, pos, eo = _tiled(env, M0)
    _, got = _both(env, 4, hdr, pos, eo, max_rows=max_rows)
    assert 6 * int(got['frontier'][3]) > lanes and got['searched_depth'][0] == 4
    assert np.array_equal(got['distance'][:REACH_N], got['distance'][-REACH_N:])
    env.reach_reserve(0, 1)
    assert env.reach_bytes == 0


# ------------------------------------------------------------------------------------------------------------------------------ 3. rows of the caller
def test_start_rows_of_the_caller():
    """tests/test_reach.py's rows: two rows of one env that differ only in step_num, 2 and 12 of max_steps 17, depth 8 -- the time-out cuts the second row's
    search; a negative env_of entry and one >= num_envs report -1, and the latter is NOT counted in expand_skipped; max_depth = 1"""
    seeds = (4017, 4031, 4013, 4029, 4004, 4117)
    env, _, _ = make_env(len(seeds), *seed_states(seeds), obs_mode='state', auto_reset=False, **K5)
    env.reset()
    envs = np.array([0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 0, 3], np.int64)
    hdr, pos = env.hdr.cpu().numpy()[envs], env.slot_pos.cpu().numpy()[envs]
    hdr[:, 8], hdr[:, 9] = np.where(np.arange(14) % 2 == 0, 2, 12), 0
    eo = envs.copy()
    eo[12], eo[13] = -3, len(seeds)
    env.seen_reserve(1 << 16)
    skipped = env.expand_skipped
    _, got = _both(env, 8, _dev(hdr), _dev(pos, np.int16), _dev(eo, np.int32), max_rows=1 << 14, engine=True)
    dist = _plans_hold(env, got, _dev(hdr), _dev(pos, np.int16), _dev(envs, np.int32))
    assert dist.tolist() == [6, -1, 7, -1, 8, -1, 3, 3, 5, 5, 2, 2, -1, -1] and got['searched_depth'][0] == 8 and got['frontier'][0] == 12
    assert env.expand_skipped == skipped
    _, got = _both(env, 1, _dev(hdr), _dev(pos, np.int16), _dev(eo, np.int32), max_rows=1 << 14)
    assert (got['distance'] == -1).all() and got['frontier'].tolist() == [12] and tuple(got['plan'].shape) == (1, 14)
    _, got = _both(env, 2, _dev(hdr), _dev(pos, np.int16), _dev(eo, np.int32), max_rows=14)         # as many start rows as max_rows
    assert got['frontier'].tolist() == [12, 0] and got['searched_depth'][0] == 1 and (got['distance'] == -1).all()   # ... and level 1 brings more than 14
    env.close()


def test_an_early_end_and_the_cap(engine5):
    """every start row one or two steps from its goal: the search ends at level 2 and the remaining levels are no-ops -- zeros in `frontier`,
    searched_depth = max_depth; and max_rows = 60 stops the twelve rows' search at level 3, with reach()'s distances"""
    env = engine5
    _, _, ref = reach_reference(5, DEPTH)
    r = env.reach(DEPTH, max_rows=1 << 14)
    dist, plan = r['distance'].cpu().numpy(), r['plan'].cpu().numpy()
    solved = np.flatnonzero(dist > 0)
    rows = np.repeat(solved, 2)
    left = np.tile([1, 2], len(solved))
    left = np.minimum(left, dist[rows])
    walk = np.full((DEPTH, len(rows)), 6, np.uint8)                                # (6: the no-op, which keeps the state)
    for k, (j, n) in enumerate(zip(rows, left)):
        walk[:dist[j] - n, k] = plan[:dist[j] - n, j]
    hdr0, pos0, eo = _dev(env.hdr.cpu().numpy()[rows]), _dev(env.slot_pos.cpu().numpy()[rows], np.int16), _dev(rows, np.int32)
    s = env.simulate(_dev(walk), hdr0, pos0, eo, fields=('hdr', 'slot_pos', 'done'))
    assert not s['done'].any()
    _, got = _both(env, 6, s['hdr'], s['slot_pos'], eo, max_rows=1 << 13)
    assert np.array_equal(got['distance'], left) and (got['frontier'][:2] > 0).all() and got['frontier'][2:].tolist() == [0] * 4
    assert got['searched_depth'][0] == 6 and set(left.tolist()) == {1, 2}
    _, got = _both(env, DEPTH, max_rows=60)
    assert got['searched_depth'][0] == 3 and got['frontier'].tolist() == [12, 35, 55] + [0] * 7
    assert np.array_equal(got['distance'], np.where((ref['distance'] > 0) & (ref['distance'] <= 3), ref['distance'], -1))


# ------------------------------------------------------------------------------------------------------------------------------ 4. repeats and capture
def test_repeats_out_and_a_set_too_small(engine5):
    env = engine5
    _, _, ref = reach_reference(5, DEPTH)
    env.seen_reserve(1 << 16)
    env.reach_reserve(1 << 14, DEPTH)
    bytes_before = env.reach_bytes
    a = env.reach_async(DEPTH)                                                     # max_rows: the workspace's
    b = env.reach_async(DEPTH)
    torch.cuda.synchronize()
    assert all(torch.equal(a[f], b[f]) for f in a) and env.reach_bytes == bytes_before and np.array_equal(a['distance'].cpu().numpy(), ref['distance'])
    _clean(env)
    for f, _ in OUT:
        a[f].view(torch.uint8).fill_(SENT)
    c = env.reach_async(DEPTH, out=a)                                              # out= (with its 'states' entry) is written again
    torch.cuda.synchronize()
    assert all(c[f] is a[f] and torch.equal(c[f], b[f]) for f, _ in OUT) and torch.equal(c['states'], b['states'])
    short = env.reach_async(4)                                                     # fewer levels than the workspace holds: no new workspace
    assert env.reach_bytes == bytes_before and tuple(short['plan'].shape) == (4, REACH_N)
    assert np.array_equal(short['distance'].cpu().numpy(), np.where((ref['distance'] > 0) & (ref['distance'] <= 4), ref['distance'], -1))
    env.seen_reserve(16)                                                           # 32 slots: nearly every row overflows, is reported fresh and expanded again
    r = env.reach_async(5)
    torch.cuda.synchronize()
    assert env.seen_overflow > 0 and r['frontier'].cpu().numpy().tolist()[0] == 12 and int(r['searched_depth'][0]) == 5
    assert np.array_equal(r['distance'].cpu().numpy(), np.where((ref['distance'] > 0) & (ref['distance'] <= 5), ref['distance'], -1))
    env.seen_reserve(1 << 20)


def test_a_spent_set_is_cleared_first(engine5):
    """the set's epochs used up (the epoch word of its control block written past CWH_SEEN_MAX_EPOCH, and a seen_insert that shows it: held keys reported
    fresh, every row counted as overflow, the epoch stuck): cw_reach clears the set before anything else, so the search that follows equals a fresh reach()
    and leaves both counters at 0"""
    from gym_craftingworld_amd import _lib as L
    from gym_craftingworld_amd._wrap import tensor_view
    env = engine5
    env.seen_reserve(1 << 12)
    p = C.c_void_p()
    assert env._lib.cw_seen_counters(env._h, C.byref(p)) == L.CW_OK
    ctl = tensor_view(p.value, (5,), torch.int64, env.device.index)                # size, overflow, collisions, EPOCH, ticket
    assert env.seen_insert(env.hdr, env.slot_pos)['fresh'].all() and int(ctl[3].item()) == 1
    ctl[3] = L.CWH_SEEN_MAX_EPOCH + 1
    again = env.seen_insert(env.hdr, env.slot_pos)
    assert again['fresh'].all() and (env.seen_size, env.seen_overflow, env.seen_collisions) == (REACH_N, REACH_N, 0)
    assert int(ctl[3].item()) == L.CWH_SEEN_MAX_EPOCH + 1                          # spent, and stuck
    out = _sentinel_out(3, REACH_N)
    r = env.reach_async(3, max_rows=1 << 10, out=out)
    torch.cuda.synchronize()
    got = _host(r)
    _clean(env)
    assert int(ctl[3].item()) == 3                                                 # (cleared, then the start rows' insert and two levels')
    check_reach_call(env.reach(3, max_rows=1 << 10), got, SENT)
    _clean(env)
    assert got['frontier'].tolist() == [12, 35, 55]
    env.seen_reserve(1 << 20)


def test_captured_into_a_graph_with_a_step():
    """torch.cuda.graph around step_many(one step) + reach_async(out=...): the calls only enqueue; each of three replays equals a fresh reach() from the
    states the envs then hold"""
    N, D = 300, 5
    env, _, _ = make_env(N, *np_states(N, 93000), obs_mode='state', auto_reset=False, **K5)
    env.reset()
    spread(env, 3, 6)
    walk_goals(env, 4, 93500)
    env.seen_reserve(1 << 17)
    env.reach_reserve(1 << 15, D)
    acts = torch.zeros((1, N), dtype=torch.uint8, device='cuda')
    out = _sentinel_out(D, N)
    env.reach_async(D, out=_sentinel_out(D, N))                                    # (warm-up outside the capture)
    env.synchronize()
    steps = int(env.counters[0])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.step_many(acts)
        r = env.reach_async(D, out=out)
    torch.cuda.synchronize()
    assert all(bool((out[f].view(torch.uint8) == SENT).all()) for f, _ in OUT) and int(env.counters[0]) == steps       # (capturing ran nothing)
    gen = torch.Generator(device='cuda').manual_seed(9)
    solved = []
    for rnd in range(3):
        acts.copy_(torch.randint(0, 6, (1, N), device='cuda', dtype=torch.uint8, generator=gen))
        g.replay()
        torch.cuda.synchronize()
        got = _host(r)
        _clean(env)
        assert int(env.counters[0]) == steps + (1 + rnd) * N
        check_reach_call(env.reach(D, max_rows=1 << 15), got, SENT)
        _clean(env)
        solved.append(int((got['distance'] > 0).sum()))
    assert min(solved) >= 5
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 5. errors
def test_call_order_and_bad_arguments():
    from gym_craftingworld_amd import CraftingWorldVecEnv, _lib as L
    env = CraftingWorldVecEnv(8, obs_mode='state', auto_reset=False, seed=3, **K5)
    lib, h, st = env._lib, env._h, env._stream()
    vp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    hdr, pos = torch.zeros((8, 16), dtype=torch.uint8, device='cuda'), torch.zeros((8, 8), dtype=torch.int16, device='cuda')
    eo = torch.zeros(8, dtype=torch.int32, device='cuda')
    out = _sentinel_out(4, 8)
    full = L.cw_reach_out(**{f: out[f].data_ptr() for f, _ in OUT})
    call = lambda *a: lib.cw_reach(*a, st)  # noqa: E731
    env.seen_reserve(64)
    env.reach_reserve(8, 4)
    assert env.reach_bytes == lib.cwh_reach_bytes_of(8, 4) > 0
    assert call(h, None, None, None, 8, 4, C.byref(full)) == L.CW_ERR_STATE and b'before cw_reset' in lib.cw_last_error()
    env.reset()
    env.seen_reserve(0)
    assert call(h, None, None, None, 8, 4, C.byref(full)) == L.CW_ERR_STATE and b'no set reserved' in lib.cw_last_error()
    env.seen_reserve(64)
    env.reach_reserve(0, 1)
    assert env.reach_bytes == 0
    assert call(h, None, None, None, 8, 4, C.byref(full)) == L.CW_ERR_STATE and b'no workspace' in lib.cw_last_error()
    env.reach_reserve(7, 4)
    assert call(h, None, None, None, 8, 4, C.byref(full)) == L.CW_ERR_STATE and b'the workspace holds 7 rows' in lib.cw_last_error()       # M0 above max_rows
    env.reach_reserve(8, 3)
    assert call(h, None, None, None, 8, 4, C.byref(full)) == L.CW_ERR_STATE and b'3 levels' in lib.cw_last_error()                         # a depth above the reserved one
    env.reach_reserve(8, 4)
    invalid = [((None, None, None, None, 8, 4, C.byref(full)), b'engine'), ((h, None, None, None, 8, 4, None), b'out'),
               ((h, None, None, None, 8, 4, C.byref(L.cw_reach_out())), b'every field'),
               ((h, None, vp(hdr), vp(pos), -1, 4, C.byref(full)), b'n_states'), ((h, None, vp(hdr), vp(pos), L.CWH_REACH_MAX_ROWS + 1, 4, C.byref(full)), b'n_states'),
               ((h, None, None, None, 8, 0, C.byref(full)), b'max_depth'), ((h, None, None, None, 8, L.CWH_REACH_MAX_DEPTH + 1, C.byref(full)), b'max_depth'),
               ((h, None, vp(hdr), None, 8, 4, C.byref(full)), b'go together'), ((h, None, None, vp(pos), 8, 4, C.byref(full)), b'go together'),
               ((h, vp(eo), None, None, 8, 4, C.byref(full)), b'env_of needs'), ((h, None, None, None, 7, 4, C.byref(full)), b'num_envs'),
               ((h, None, vp(hdr, 8), vp(pos), 7, 4, C.byref(full)), b'aligned'), ((h, None, vp(hdr), vp(pos, 2), 7, 4, C.byref(full)), b'aligned'),
               ((h, vp(eo, 2), vp(hdr), vp(pos), 7, 4, C.byref(full)), b'aligned'),
               ((h, None, vp(hdr), vp(pos), 7, 4, C.byref(L.cw_reach_out(distance=out['distance'].data_ptr() + 2))), b'aligned'),
               ((h, None, vp(hdr), vp(pos), 8, 4, C.byref(L.cw_reach_out(plan=hdr.data_ptr() + 127))), b'overlaps'),
               ((h, vp(eo), vp(hdr), vp(pos), 8, 4, C.byref(L.cw_reach_out(frontier=eo.data_ptr() + 16))), b'overlaps'),
               ((h, None, vp(hdr), vp(pos), 8, 4, C.byref(L.cw_reach_out(distance=out['distance'].data_ptr(), first_action=out['distance'].data_ptr() + 31))),
                b'overlaps')]
    for args, word in invalid:
        assert call(*args) == L.CW_ERR_INVALID, word
        assert word in lib.cw_last_error(), (word, lib.cw_last_error())
    for bad in ((-1, 4), (L.CWH_REACH_MAX_ROWS + 1, 4), (8, 0), (8, L.CWH_REACH_MAX_DEPTH + 1)):
        assert lib.cw_reach_reserve(h, *bad) == L.CW_ERR_INVALID
        with pytest.raises(ValueError):
            env.reach_reserve(*bad)
    torch.cuda.synchronize()
    assert all(bool((out[f].view(torch.uint8) == SENT).all()) for f, _ in OUT) and env.reach_bytes == lib.cwh_reach_bytes_of(8, 4)
    for bad in (dict(max_depth=0), dict(max_depth=2.0), dict(max_depth=4, max_rows=0), dict(max_depth=4, max_rows=7), dict(max_depth=4, hdr=hdr),
                dict(max_depth=4, env_of=eo), dict(max_depth=4, out={'distance': out['distance']}), dict(max_depth=3, out=out),
                dict(max_depth=4, out=dict(out, distance=out['distance'].to(torch.int64)))):
        with pytest.raises(ValueError):
            env.reach_async(**bad)
    with pytest.raises(IndexError):
        env.reach_async(4, hdr.cpu().numpy(), pos.cpu().numpy(), [0, 1, 2, 3, 4, 5, 6, 8])          # the host-validated path names an env outside the batch
    env.reach_reserve(0, 1)
    env.seen_reserve(0)
    r = env.reach_async(2, env.hdr.cpu().numpy(), env.slot_pos.cpu().numpy(), [0, 1, 2, -1, 4, 5, 6, 7], max_rows=100)     # reserves both: a set for 400 keys, 100 rows
    torch.cuda.synchronize()
    assert env.seen_slots == 1024 and env.reach_bytes == lib.cwh_reach_bytes_of(100, 2) and r['frontier'].cpu().numpy()[0] == 7
    assert r['distance'].cpu().numpy()[3] == -1
    env.close()
