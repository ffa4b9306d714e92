"""GPU tier of whole trajectories: cw_unroll_kernel through CraftingWorldVecEnv.unroll.  Every call is checked row by row with unroll_check.check_unroll
(itself tested on the CPU, tests/test_unroll_logic.py): every written row at every t against a chain of one-step oracle calls, every row that must not be
written against a sentinel, and the engine before and after the call byte for byte; and against the sibling calls -- simulate(), chained expand(), the
engine's own step(), render_records() -- on packed bytes.  Everything is bit-exact.  No timing."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from engines import ENGINES, K5, N1, k_of
from masked_check import spread, take
from oracle_replay import make_env, np_states
from records_check import POS_GONE, POS_HELD, decode, oracle_simulate
from records_gpu import SENT, caller_records, dev as _dev, env_of_cases, host as _host, sentinel_out, walked_engine
from simulate_check import RECIPE_KW, RECIPE_N, recipe
from state_tables import painted_batch
from unroll_check import FIELDS, TRACES, check_unroll, layout, oracle_unroll

pytestmark = pytest.mark.gpu

BLOCK = 8                                       # CW_SIM_BLOCK: the action bytes are fetched this many steps at a time
_WIDTH = dict(hdr=16, slot_pos=16, reward=4, done=1, changed=1, taken=1, length=4)
_DTYPE = dict(hdr=torch.uint8, slot_pos=torch.int16, reward=torch.int32, done=torch.bool, changed=torch.bool, taken=torch.bool, length=torch.int32)


def _sentinel_out(T, M, fields=FIELDS):
    """output buffers as unroll(out=...) takes them, every byte SENT"""
    return sentinel_out({f: layout(T)[f] for f in fields}, _WIDTH, _DTYPE, M)


def _dense_of(snap, rows=None):
    d = decode(snap['hdr'], snap['slot_pos'], snap['state_grid'].shape[1])
    return {k: (v if rows is None else v[rows]) for k, v in d.items()}


def _plans(seed, T, M, noops=0.0):
    """actions uint8 [T, M]: 0..5, and with probability `noops` one of the ids 6, 200, 255 (the state-preserving no-op)"""
    rng = np.random.RandomState(seed)
    a = rng.randint(0, 6, (T, M)).astype(np.uint8)
    if noops:
        on = rng.rand(T, M) < noops
        a[on] = rng.choice([6, 200, 255], int(on.sum()))
    return a


def _near_goals(states, init_grids, acts, okw, steps, every=2):
    """desired of every `every`-th state := the achieved mask the oracle reaches after `steps` steps of the state's own plan: goals that get satisfied"""
    reached = oracle_simulate(states, init_grids, acts[:steps], False, okw)['achieved']
    return np.where(np.arange(len(reached)) % every == 0, reached, np.asarray(states['desired']))


def _reachable_goals(env, acts, okw, steps):
    """_near_goals on the engine's own states, plan column i being env i's -> the snapshot after desired was set"""
    before = take(env)
    env.set_state(desired=_near_goals(_dense_of(before), before['state_init_grid'], acts[:, :env.num_envs], okw, steps).astype(np.uint16))
    return take(env)


# ------------------------------------------------------------------------------------------------------------------------------ 1. the shared batch of plans
def _recipe_engine(style):
    dense, _, _ = recipe(12, style)
    env, _, _ = make_env(RECIPE_N, *np_states(RECIPE_N, 900), obs_mode='state', reward_style=style, auto_reset=False, **RECIPE_KW)
    env.reset()
    env.set_state(desired=dense['desired'].astype(np.uint16))
    before = take(env)
    flags = _dense_of(before)['flags']
    assert ((flags & ~1) == (2 if style else 0)).all()
    return env, before, flags


@functools.lru_cache(maxsize=None)
def _recipe_want(T, style, stop, flags):
    dense, init_grids, acts = recipe(T, style)
    states = dict(dense, flags=np.array(flags))
    return states, oracle_unroll(states, init_grids, acts, stop, RECIPE_KW)


@pytest.mark.parametrize('stop', [True, False])
@pytest.mark.parametrize('style', [None, 'subset'])
@pytest.mark.parametrize('T', [12, 24])
def test_the_recipe_against_the_oracle(T, style, stop):
    """600 plans that never end, end by success and end by time-out (simulate_check.recipe), the records handed in through hdr= / slot_pos=; all seven
    fields, under both reward rules and both stop rules"""
    env, before, flags = _recipe_engine(style)
    acts = recipe(T, style)[2]
    states, want = _recipe_want(T, style, stop, tuple(flags.tolist()))
    ended = (want['taken'].sum(axis=0) < T).sum()
    assert ended >= 200 if stop else ended == 0
    n = int(want['changed'].sum())
    assert n >= 1000 and want['changed'].size - n >= 1000
    if T == 12 and not stop and style is None:
        assert n == 3666
    out = _sentinel_out(T, RECIPE_N)
    r = env.unroll(_dev(acts), hdr=env.hdr.clone(), slot_pos=env.slot_pos.clone(), stop_at_done=stop, out=out)
    assert list(r) == list(FIELDS) and all(r[f] is out[f] for f in FIELDS)
    part, skipped = check_unroll(before, take(env), dict(hdr=before['hdr'], slot_pos=before['slot_pos']), None, acts, stop, _host(out), SENT,
                                 oracle_kw=RECIPE_KW, expected=(states, want))
    assert (part, skipped) == (RECIPE_N, 0)
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 2. block edges of the action prefetch
@pytest.fixture(scope='module')
def engine70():
    env = walked_engine(81000, 6)
    yield env
    env.close()


@pytest.mark.parametrize('stop', [True, False])
@pytest.mark.parametrize('T', [1, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK, 2 * BLOCK + 1])
def test_horizons_around_the_action_block(engine70, T, stop):
    """T = 1, 7, 8, 9, 16, 17 on the engine's own states after a spread (held and vanished slots), two plans per env, goals within reach, the no-op ids 6,
    200 and 255 mixed in"""
    env = engine70
    acts = _plans(200 + T, T, 2 * N1, noops=0.15)
    acts[0, :3] = [6, 200, 255]
    before = _reachable_goals(env, acts, K5, min(T, 3))
    p = before['slot_pos'].view(np.uint16)
    assert (p == POS_HELD).any() and (p == POS_GONE).any()
    out = _sentinel_out(T, 2 * N1)
    env.unroll(_dev(acts), stop_at_done=stop, out=out)
    got = _host(out)
    part, _ = check_unroll(before, take(env), None, None, acts, stop, got, SENT, oracle_kw=K5)
    assert part == 2 * N1 and (got['reward'] == K5['max_steps']).any()
    noop = acts > 5
    assert noop[got['taken'] == 1].sum() >= 3 and not got['changed'][noop].any() and (got['reward'][noop & (got['taken'] == 1)] == -1).all()


# ------------------------------------------------------------------------------------------------------------------------------ 3. a wave that leaves early, the tail loop
@pytest.mark.parametrize('style,counted', [(None, (292, 302)), ('subset', (294, 299))])
def test_a_workgroup_that_leaves_at_the_first_block_boundary(style, counted):
    """the recipe at T = 16, its columns permuted so that the first 256 are states whose plan ends within 8 steps: waves 0-3 leave at the block boundary 8
    and rows 9 .. 16 come from the tail loop, while other waves run all 16 steps.  The records go in permuted, env_of = the permutation."""
    T = 2 * BLOCK
    env, before, flags = _recipe_engine(style)
    acts = recipe(T, style)[2]
    states, want = _recipe_want(T, style, True, tuple(flags.tolist()))
    early, never = np.flatnonzero(want['length'] <= BLOCK), np.flatnonzero(~want['done'].any(axis=0))
    assert (len(early), len(never)) == counted and len(early) >= 256
    perm = np.concatenate([early[:256], np.setdiff1d(np.arange(RECIPE_N), early[:256])])
    assert (want['taken'][BLOCK:, perm[:256]] == 0).all() and want['taken'][T - 1, perm[256:]].sum() >= 256
    hdr, pos, a = before['hdr'][perm], before['slot_pos'][perm], np.ascontiguousarray(acts[:, perm])
    out = _sentinel_out(T, RECIPE_N)
    env.unroll(_dev(a), _dev(hdr), _dev(pos, np.int16), _dev(perm, np.int32), out=out)
    sub = {k: (v[:, perm] if v.ndim > 1 else v[perm]) for k, v in want.items()}
    check_unroll(before, take(env), dict(hdr=hdr, slot_pos=pos), perm, a, True, _host(out), SENT, oracle_kw=RECIPE_KW,
                 expected=({k: v[perm] for k, v in states.items()}, sub))
    assert torch.equal(out['hdr'][BLOCK + 1:, :256], out['hdr'][BLOCK:BLOCK + 1, :256].expand(T - BLOCK, 256, 16))      # the frozen record repeated by the tail
    assert not out['taken'][BLOCK:, :256].any() and not out['reward'][BLOCK:, :256].any()
    env.close()


def test_every_wave_leaves_and_the_tail_writes_the_clamped_last_block():
    """T = 33 on the unpermuted recipe: every state has ended by step 17 (max_steps, fresh states), every wave leaves at boundary 24, and rows 25 .. 33
    come from the tail loop, behind a last prefetched block clamped to row 32"""
    T = 4 * BLOCK + 1
    env, before, flags = _recipe_engine(None)
    acts = recipe(T, None)[2]
    states, want = _recipe_want(T, None, True, tuple(flags.tolist()))
    assert (want['length'] <= RECIPE_KW['max_steps']).all() and want['done'].any(axis=0).all()
    out = _sentinel_out(T, RECIPE_N)
    env.unroll(_dev(acts), hdr=env.hdr.clone(), slot_pos=env.slot_pos.clone(), out=out)
    check_unroll(before, take(env), dict(hdr=before['hdr'], slot_pos=before['slot_pos']), None, acts, True, _host(out), SENT, oracle_kw=RECIPE_KW,
                 expected=(states, want))
    assert not out['taken'][17:].any() and torch.equal(out['slot_pos'][18:], out['slot_pos'][17:18].expand(T - 17, RECIPE_N, 8))
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 4. against the sibling calls, on packed bytes
@pytest.mark.parametrize('stop', [True, False])
def test_against_simulate_and_chained_expand(engine70, stop):
    """simulate() of the same arguments: the final records, the traces and length; expand() chained: row t + 1 is row (a_t, j) of expand(row t), with its
    `changed`, for every step taken with an action id <= 5 -- bytes, not decoded states"""
    env, T, M = engine70, BLOCK + 3, 3 * N1
    acts = _plans(300 + stop, T, M, noops=0.1)
    _reachable_goals(env, acts, K5, 3)
    t_acts = _dev(acts)
    r = env.unroll(t_acts, stop_at_done=stop)
    s = env.simulate(t_acts, stop_at_done=stop, fields=('hdr', 'slot_pos', 'rewards', 'dones', 'length', 'achieved_mask'))
    assert torch.equal(r['hdr'][T], s['hdr']) and torch.equal(r['slot_pos'][T], s['slot_pos'])
    assert torch.equal(r['reward'], s['rewards']) and torch.equal(r['done'], s['dones']) and torch.equal(r['length'], s['length'])
    assert torch.equal(r['hdr'][T][:, 4:6].contiguous().view(torch.int16).squeeze(-1), s['achieved_mask'])      # (the achieved mask: bytes 4-5 of the header)
    assert torch.equal(r['hdr'][0], env.hdr.repeat(3, 1)) and torch.equal(r['slot_pos'][0], env.slot_pos.repeat(3, 1))      # row 0: the records tiled
    cols, env_of = torch.arange(M, device='cuda'), (torch.arange(M, device='cuda') % N1).to(torch.int32)
    assert r['done'].any() and (r['taken'].all() if not stop else not r['taken'].all())
    compared = 0
    for t in range(T):
        e = env.expand(hdr=r['hdr'][t], slot_pos=r['slot_pos'][t], env_of=env_of)
        a = t_acts[t].long()
        on = r['taken'][t] & (a <= 5)
        a = a.clamp(max=5)
        assert torch.equal(r['hdr'][t + 1][on], e['hdr'][a, cols][on]) and torch.equal(r['slot_pos'][t + 1][on], e['slot_pos'][a, cols][on]), t
        assert torch.equal(r['changed'][t][on], e['changed'][a, cols][on]) and torch.equal(r['reward'][t][on], e['reward'][a, cols][on]), t
        off = ~r['taken'][t]
        assert torch.equal(r['hdr'][t + 1][off], r['hdr'][t][off]) and torch.equal(r['slot_pos'][t + 1][off], r['slot_pos'][t][off]), t
        compared += int(on.sum())
    assert compared >= T * M // 2


def test_against_the_engines_own_step_on_packed_bytes():
    """unroll(stop_at_done=False) first, then the same T steps by step() on an auto_reset=False engine mid-episode: env.hdr / env.slot_pos after step t
    are row t + 1, byte for byte; reward and done are what the steps returned"""
    T = 12
    env, _, _ = make_env(N1, *np_states(N1, 82000), **ENGINES['state_manual'], **K5)
    env.reset()
    spread(env, 9, 2)
    acts = _plans(63, T, N1)
    before = _reachable_goals(env, acts, K5, 3)
    assert (before['state_step_num'] > 0).any()
    t_acts = _dev(acts)
    r = env.unroll(t_acts, stop_at_done=False)
    check_unroll(before, take(env), None, None, acts, False, _host(r), SENT, oracle_kw=K5)
    assert torch.equal(r['hdr'][0], env.hdr) and torch.equal(r['slot_pos'][0], env.slot_pos)
    for t in range(T):
        _, rew, done, _ = env.step(t_acts[t])
        assert torch.equal(env.hdr, r['hdr'][t + 1]) and torch.equal(env.slot_pos, r['slot_pos'][t + 1]), t
        assert torch.equal(rew.to(torch.int32), r['reward'][t]) and torch.equal(done.to(torch.bool), r['done'][t]), t
    assert r['done'].any() and (r['reward'] == K5['max_steps']).any() and r['taken'].all()
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 5. who takes part
def _edge_call(env, M, T, stop, seed, fields=FIELDS, with_env_of=True, bufs=None):
    before = take(env)
    if with_env_of:
        e = env_of_cases(M, N1) if M >= 63 else np.random.RandomState(seed).randint(0, N1, M).astype(np.int64)
    else:
        e = None
    hdr, pos = caller_records(before, np.arange(M) % N1 if e is None else e, M, N1, K5['max_steps'])
    acts = _plans(seed, T, M, noops=0.08)
    bufs = bufs or _sentinel_out(T, M, fields)
    out = {f: bufs[f] for f in fields}
    skipped0 = env.expand_skipped
    r = env.unroll(_dev(acts), _dev(hdr), _dev(pos, np.int16), None if e is None else _dev(e, np.int32), stop_at_done=stop, fields=fields, out=out)
    assert list(r) == list(fields)
    part, skipped = check_unroll(before, take(env), dict(hdr=hdr, slot_pos=pos), e, acts, stop, _host(out), SENT, oracle_kw=K5)
    assert env.expand_skipped == skipped0 + skipped
    return e, part, skipped, out


@pytest.mark.parametrize('M', [5, 63, 64, 65, 257])
def test_who_takes_part(engine70, M):
    """caller records with M < N and M > N around the wave and the workgroup; from 63 states on env_of mixes valid ids, repeats, -1, -7, N, N + 31 and
    INT32_MAX: every one of the T + 1 / T / 1 rows of those states still holds the sentinel, and counters[7] rises once per skipped state"""
    e, part, skipped, _ = _edge_call(engine70, M, BLOCK + 1, True, 100 + M)
    assert part == int(((e >= 0) & (e < N1)).sum()) and skipped == int((e >= N1).sum())
    if M >= 63:
        assert skipped >= 3 and (e < 0).sum() >= 2
    _, part, skipped, _ = _edge_call(engine70, M, 3, False, 150 + M, with_env_of=False)       # env_of == NULL: record j is env j % N's
    assert (part, skipped) == (M, 0)


def test_the_broadcast_form(engine70):
    """actions [T, 3, N] with no records handed in: state k * N + i is env i's"""
    env, T, K = engine70, 5, 3
    acts = _plans(160, T, K * N1, noops=0.05)
    before = take(env)
    out = _sentinel_out(T, K * N1)
    env.unroll(_dev(acts).reshape(T, K, N1), out=out)
    part, _ = check_unroll(before, take(env), None, None, acts.reshape(T, K, N1), True, _host(out), SENT, oracle_kw=K5)
    assert part == K * N1 and tuple(out['hdr'].shape) == (T + 1, K * N1, 16)
    flat = env.unroll(acts)                                       # the host path, [T, K * N]
    assert all(torch.equal(flat[f], out[f]) for f in FIELDS)


def test_no_states(engine70):
    r = engine70.unroll(torch.empty((5, 0), dtype=torch.uint8, device='cuda'), hdr=torch.empty((0, 16), dtype=torch.uint8, device='cuda'),
                        slot_pos=torch.empty((0, 8), dtype=torch.int16, device='cuda'))
    assert set(r) == set(FIELDS) and tuple(r['reward'].shape) == (5, 0) and tuple(r['hdr'].shape) == (6, 0, 16)


# ------------------------------------------------------------------------------------------------------------------------------ 6. every engine kind
KINDS = dict(ENGINES, host_outputs=dict(obs_mode='pixels_dirty', host_outputs=True, auto_reset=False))


@pytest.fixture(scope='module')
def shared_call():
    """records and plans every engine kind is handed alike, and what the plain state engine makes of them"""
    T = BLOCK + 2
    env, _, _ = make_env(N1, *np_states(N1, 83000), **ENGINES['state_manual'], **K5)
    env.reset()
    before = take(env)
    acts = _plans(170, T, 2 * N1, noops=0.05)
    walk = env.simulate(_dev(_plans(171, 4, 2 * N1)), stop_at_done=False, fields=('hdr', 'slot_pos'))      # records four steps into the envs' episodes
    hdr, pos = walk['hdr'].cpu().numpy(), walk['slot_pos'].cpu().numpy()
    ref = _host(env.unroll(_dev(acts), _dev(hdr), _dev(pos, np.int16)))
    env.close()
    return T, acts, hdr, pos, before['state_init_grid'], ref


@pytest.mark.parametrize('kind', list(KINDS))
def test_every_engine_kind(shared_call, kind):
    """the three obs modes, with and without auto-reset, host_outputs: the engine's own states against the oracle with every buffer, stream, frame and
    counter untouched; and the shared records give the same bytes on every kind whose envs started where the plain engine's did"""
    T, acts, hdr, pos, init_grid, ref = shared_call
    n = 4 if kind == 'host_outputs' else N1
    ekw = dict(KINDS[kind])
    if 'env_menu' in ekw:
        ekw['env_menu'] = ekw['env_menu'][:n]
    env, _, _ = make_env(n, *np_states(n, 83000), **ekw, **K5)
    env.reset()
    fresh = take(env)
    if np.array_equal(fresh['state_init_grid'], init_grid[:n]) and 'task_menus' not in ekw:
        m = 2 * N1 if n == N1 else 2 * n
        e = None if n == N1 else _dev(np.arange(m) % n, np.int32)
        cols = np.arange(m) if n == N1 else np.concatenate([np.arange(n), N1 + np.arange(n)])
        got = _host(env.unroll(_dev(np.ascontiguousarray(acts[:, cols])), _dev(hdr[cols]), _dev(pos[cols], np.int16), e))
        for f in FIELDS:
            assert np.array_equal(got[f], ref[f][cols] if f == 'length' else ref[f][:, cols]), (f, kind)
    else:
        assert kind == 'state_auto_pool_menus'                    # (a pool of start states and menus of its own: other episodes)
    if env.host_outputs:
        for a in (1, 2, 4, 1, 5, 0):
            env.step(np.full(n, a, np.int32))
    else:
        spread(env, 7, 4)
    before = take(env)
    if env.obs_mode != 'state':
        assert 'observation' in before and 'desired_goal' in before
    out = _sentinel_out(T, 2 * n)
    a = np.ascontiguousarray(acts[:, :2 * n])
    r = env.unroll(a if env.host_outputs else _dev(a), out=out)
    assert all(r[f] is out[f] and r[f].is_cuda for f in FIELDS)
    part, _ = check_unroll(before, take(env), None, None, a, True, _host(out), SENT, oracle_kw=K5)
    assert part == 2 * n
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 7. a large grid
def test_a_large_grid():
    """255 x 255, N = 9, T = 9: slot cells above 32 767 (negative in the int16 tensors), rows and columns above 127"""
    S, N, K, T = 255, 9, 2, BLOCK + 1
    okw = k_of(S)
    _, grid, init, agent, hold = painted_batch(S, 22)
    far = [j for j in range(22) if max(agent[j]) >= 128][:N]
    assert len(far) == N
    grid, init, agent, hold = grid[far], init[far], agent[far], hold[far]
    env, _, _ = make_env(N, *np_states(N, 84000), obs_mode='state', auto_reset=False, **okw)
    env.reset()
    env.set_state(grid=grid, init_grid=init, agent_rc=agent, init_agent_rc=agent, hold=hold, step_num=np.full(N, okw['max_steps'] - 6, np.int32))
    acts = _plans(68, T, K * N)
    before = _reachable_goals(env, acts, okw, 2)
    above = int(((before['slot_pos'].view(np.uint16) > 32767) & (before['slot_pos'].view(np.uint16) < POS_HELD)).sum())
    assert above >= N and (before['slot_pos'] < -2).sum() == above
    for stop in (True, False):
        out = _sentinel_out(T, K * N)
        env.unroll(_dev(acts), stop_at_done=stop, out=out)
        part, _ = check_unroll(before, take(env), None, None, acts, stop, _host(out), SENT, oracle_kw=okw)
        assert part == K * N
    assert out['done'].any() and (out['slot_pos'][1:].cpu().numpy() < -2).any() and (out['hdr'][1:, :, :2] >= 128).any()
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 8. field subsets
@pytest.mark.parametrize('fields', [(f,) for f in FIELDS] + [('hdr', 'slot_pos'), ('taken', 'hdr'), TRACES])
def test_subsets_of_the_fields(engine70, fields):
    """each field alone, hdr without slot_pos and the reverse, the traces alone: the buffers of the fields not named keep their sentinel"""
    T, M = BLOCK + 1, 65
    bufs = _sentinel_out(T, M)
    _, part, _, out = _edge_call(engine70, M, T, True, 400, fields=fields, bufs=bufs)
    assert set(out) == set(fields) and part > 50
    torch.cuda.synchronize()
    for f in FIELDS:
        if f not in fields:
            assert bool((bufs[f].view(torch.uint8) == SENT).all()), f


# ------------------------------------------------------------------------------------------------------------------------------ 9. capture
def test_captured_into_a_graph():
    """torch.cuda.graph around one unroll(out=...) on one stream: the call only enqueues; replayed twice, the action tensor refilled in place between the
    replays, each replay equals the eager call"""
    N, K, T = 300, 2, BLOCK + 1
    env, _, _ = make_env(N, *np_states(N, 85000), obs_mode='state', **K5)
    env.reset()
    spread(env, 5, 6)
    acts = _dev(_plans(7, T, K * N))
    out = _sentinel_out(T, K * N)
    env.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.unroll(acts, out=out)
    assert all(bool((t.view(torch.uint8) == SENT).all()) for t in out.values())          # (capturing ran nothing)
    for rnd in range(2):
        acts.copy_(_dev(_plans(8 + rnd, T, K * N, noops=0.05)))
        g.replay()
        eager = env.unroll(acts)
        for f in FIELDS:
            assert torch.equal(out[f], eager[f]), (rnd, f)
    before = take(env)
    g.replay()
    torch.cuda.synchronize()
    check_unroll(before, take(env), None, None, acts.cpu().numpy(), True, _host(out), SENT, oracle_kw=K5)
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 10. with render_records
def test_the_frames_of_the_steps_taken_in_one_render_records_call():
    """8 envs on a pixels_dirty engine without auto-reset, T = 6: rows 1 .. T painted in ONE render_records call with mask = taken are the frames the
    engine shows after each step(); the frame of a step not taken is not written"""
    N, T = 8, 6
    env, _, _ = make_env(N, *np_states(N, 86000), obs_mode='pixels_dirty', auto_reset=False, **K5)
    env.reset()
    spread(env, 4, 5)
    acts = _plans(87, T, N)
    sn = env.get_state()['step_num'].copy()
    sn[1::2] = K5['max_steps'] - 3                                # every other env three steps before the time-out: plans that end early
    env.set_state(step_num=sn)
    _reachable_goals(env, acts, K5, 2)
    t_acts = _dev(acts)
    r = env.unroll(t_acts)
    taken = r['taken'].clone()
    assert taken[0].all() and (~taken[T - 1]).sum() >= N // 2
    frames = torch.full((T * N,) + tuple(env.frame_shape), SENT, dtype=torch.uint8, device='cuda')
    got = env.render_records(r['hdr'][1:].reshape(-1, 16), r['slot_pos'][1:].reshape(-1, 8), mask=r['taken'].reshape(-1), out=frames)
    got = got.reshape((T, N) + tuple(env.frame_shape))
    for t in range(T):
        obs, _, _, _ = env.step(t_acts[t])
        on = taken[t]
        assert torch.equal(got[t][on], obs['observation'][on]), t
        assert bool((got[t][~on] == SENT).all()), t
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 11. the entry point through ctypes
def test_call_order_and_arguments_through_ctypes():
    from gym_craftingworld_amd import CraftingWorldVecEnv, _lib as L
    N, T = 8, 3
    env = CraftingWorldVecEnv(N, obs_mode='state', auto_reset=False, seed=3, **K5)
    lib, h, st = env._lib, env._h, env._stream()
    bufs = _sentinel_out(T, N)
    acts = _dev(_plans(6, T, N))
    vp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    one = lambda **kw: L.cw_unroll_out(**kw)  # noqa: E731
    full = one(**{f: vp(bufs[f]) for f in FIELDS})
    with pytest.raises(L.CraftingWorldError):                                      # before reset(), through the method
        env.unroll(acts)
    assert lib.cw_unroll(h, None, None, None, N, vp(acts), T, 1, C.byref(full), st) == L.CW_ERR_STATE and b'before cw_reset' in lib.cw_last_error()
    env.reset()
    hdr, pos, eo = vp(env.hdr), vp(env.slot_pos), torch.zeros(N + 1, dtype=torch.int32, device='cuda')
    ch, cp = env.hdr.clone(), env.slot_pos.clone()
    assert lib.cw_unroll(h, None, None, None, N, vp(acts), T, 1, C.byref(full), st) == L.CW_OK
    assert lib.cw_unroll(h, None, vp(ch), vp(cp), 0, vp(acts), T, 1, C.byref(full), st) == L.CW_OK         # no states: nothing enqueued
    a = vp(acts)
    big = torch.zeros(16 * (T + 2) * N, dtype=torch.uint8, device='cuda')          # room for adjacent outputs
    rec = 16 * (T + 1) * N
    adjacent = one(hdr=vp(bufs['hdr']), slot_pos=vp(bufs['slot_pos']), reward=vp(big), done=vp(big, 4 * T * N), changed=vp(big, 5 * T * N),
                   taken=vp(big, 6 * T * N), length=vp(big, 8 * T * N))
    assert lib.cw_unroll(h, None, vp(ch), vp(cp), N, a, T, 1, C.byref(adjacent), st) == L.CW_OK, lib.cw_last_error()      # adjacent, not overlapping
    both = torch.zeros(2 * 16 * N + rec, dtype=torch.uint8, device='cuda')         # ... the records read and the rows written back to back
    assert lib.cw_unroll(h, None, vp(both), vp(both, 16 * N), N, a, T, 1, C.byref(one(hdr=vp(both, 32 * N))), st) == L.CW_OK, lib.cw_last_error()
    invalid = [((None, None, None, None, N, a, T, 1, C.byref(full)), b'engine'),
               ((h, None, None, None, N, a, T, 1, None), b'out'),
               ((h, None, None, None, N, None, T, 1, C.byref(full)), b'actions'),
               ((h, None, None, None, N, a, T, 1, C.byref(one())), b'every field'),
               ((h, None, vp(ch), vp(cp), -1, a, T, 1, C.byref(full)), b'n_states'),
               ((h, None, vp(ch), vp(cp), 2 ** 27 + 1, a, T, 1, C.byref(full)), b'n_states'),
               ((h, None, None, None, N, a, 0, 1, C.byref(full)), b'n_steps'),
               ((h, None, None, None, N, a, 32768, 1, C.byref(full)), b'n_steps'),
               ((h, None, vp(ch), None, 2 ** 26, a, 2, 1, C.byref(full)), b'records in one call'),            # (the cap comes before the pointer rules)
               ((h, None, None, None, N - 1, a, T, 1, C.byref(full)), b'multiple of num_envs'),
               ((h, None, vp(ch), None, N, a, T, 1, C.byref(full)), b'hdr_in given without slot_pos_in'),
               ((h, None, None, vp(cp), N, a, T, 1, C.byref(full)), b'slot_pos_in given without hdr_in'),
               ((h, vp(eo), None, None, N, a, T, 1, C.byref(full)), b'env_of'),
               ((h, None, vp(ch, 8), vp(cp), N - 1, a, T, 1, C.byref(full)), b'hdr_in is not 16-byte aligned'),          # each misalignment
               ((h, None, vp(ch), vp(cp, 2), N - 1, a, T, 1, C.byref(full)), b'slot_pos_in is not 16-byte aligned'),
               ((h, None, vp(ch), vp(cp), N - 1, a, T, 1, C.byref(one(hdr=vp(bufs['hdr'], 4)))), b'out->hdr is not 16-byte aligned'),
               ((h, None, vp(ch), vp(cp), N - 1, a, T, 1, C.byref(one(slot_pos=vp(bufs['slot_pos'], 8)))), b'out->slot_pos is not 16-byte aligned'),
               ((h, None, vp(ch), vp(cp), N - 1, a, T, 1, C.byref(one(reward=vp(bufs['reward'], 2)))), b'out->reward is not 4-byte aligned'),
               ((h, None, vp(ch), vp(cp), N - 1, a, T, 1, C.byref(one(length=vp(bufs['length'], 1)))), b'out->length is not 4-byte aligned'),
               ((h, vp(eo, 2), vp(ch), vp(cp), N, a, T, 1, C.byref(full)), b'env_of is not 4-byte aligned'),
               ((h, None, vp(ch), vp(cp), N, a, T, 1, C.byref(one(hdr=vp(ch)))), b'out->hdr overlaps the records read'),            # each overlap class
               ((h, None, vp(ch), vp(cp), N - 1, a, T, 1, C.byref(one(slot_pos=vp(cp, 16 * (N - 2))))), b'out->slot_pos overlaps the records read'),
               ((h, None, None, None, N, a, T, 1, C.byref(one(hdr=hdr))), b'out->hdr overlaps the records read'),                 # (the engine's own)
               ((h, None, None, None, 2 * N, a, T, 1, C.byref(one(slot_pos=pos))), b'out->slot_pos overlaps the records read'),
               ((h, None, None, None, N, a, T, 1, C.byref(one(done=vp(acts, T * N - 1)))), b'out->done overlaps actions'),
               ((h, None, None, None, N, a, T, 1, C.byref(one(taken=a))), b'out->taken overlaps actions'),
               ((h, vp(eo), vp(ch), vp(cp), N, a, T, 1, C.byref(one(length=vp(eo, 4)))), b'out->length overlaps env_of'),
               ((h, None, None, None, N, a, T, 1, C.byref(one(reward=vp(big), changed=vp(big, 4 * T * N - 1)))), b'out->reward overlaps out->changed'),
               ((h, None, None, None, N, a, T, 1, C.byref(one(hdr=vp(bufs['hdr']), slot_pos=vp(bufs['hdr'], rec - 16)))), b'out->hdr overlaps out->slot_pos'),
               ((h, None, None, None, N, a, T, 1, C.byref(one(done=vp(big), taken=vp(big)))), b'out->done overlaps out->taken')]
    for args, word in invalid:
        assert lib.cw_unroll(*args, st) == L.CW_ERR_INVALID, word
        assert word in lib.cw_last_error(), (word, lib.cw_last_error())
    torch.cuda.synchronize()
    assert env.expand_skipped == 0
    env.close()
