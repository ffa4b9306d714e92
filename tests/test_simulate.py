"""GPU tier of trying plans: cw_simulate_kernel through CraftingWorldVecEnv.simulate.  Every call is checked row by row with simulate_check.check_simulate
(itself tested on the CPU, tests/test_simulate_logic.py): every written row against the CPU oracle's set_state + T x step, every row that must not be
written -- trace rows included -- against a sentinel, and the engine before and after the call byte for byte.  Everything is bit-exact.  No timing."""
import ctypes as C

import numpy as np
import pytest
import torch

from engines import ENGINES, K5, N1, SIZES, k_of
from masked_check import spread, take
from oracle_replay import make_env, np_states, record_steps, same
from records_check import DENSE, POS_GONE, POS_HELD, decode, oracle_simulate
from records_gpu import SENT, caller_records, dev as _dev, env_of_cases, host as _host, sentinel_out, walked_engine
from simulate_check import FIELDS, RECIPE_KW, RECIPE_N, TRACES, assert_recipe_coverage, check_simulate, coverage, layout, recipe
from state_tables import painted_batch, wall_table

pytestmark = pytest.mark.gpu

BLOCK = 8                                       # CW_SIM_BLOCK: the action bytes are fetched this many steps at a time
_WIDTH = dict(ret=4, length=4, done=1, achieved_mask=2, hdr=16, slot_pos=16, rewards=4, dones=1)
_DTYPE = dict(ret=torch.int32, length=torch.int32, done=torch.bool, achieved_mask=torch.int16, hdr=torch.uint8, slot_pos=torch.int16, rewards=torch.int32,
              dones=torch.bool)


def _sentinel_out(T, M, fields=FIELDS):
    """output buffers as simulate(out=...) takes them, every byte SENT"""
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


# ------------------------------------------------------------------------------------------------------------------------------ 1. the shared batch of plans
@pytest.fixture(scope='module')
def recipe_coverage():
    """what the recipe exercises under each reward rule, counted from the oracle alone and asserted before anything is compared"""
    cov = {}
    for style in (None, 'subset'):
        cov[style] = [coverage(oracle_simulate(*recipe(T, style), False, RECIPE_KW), RECIPE_KW['max_steps']) for T in (12, 24)]
        assert_recipe_coverage(*cov[style])
    return cov


@pytest.mark.parametrize('stop', [True, False])
@pytest.mark.parametrize('style', [None, 'subset'])
@pytest.mark.parametrize('T', [12, 24])
def test_the_recipe_against_the_oracle(recipe_coverage, T, style, stop):
    """600 plans that never end, end by success and end by time-out (simulate_check.recipe), the records handed in through hdr= / slot_pos=; all eight
    fields, under both reward rules and both stop rules"""
    dense, init_grids, acts = recipe(T, style)
    env, _, _ = make_env(RECIPE_N, *np_states(RECIPE_N, 900), obs_mode='state', reward_style=style, auto_reset=False, **RECIPE_KW)
    env.reset()
    env.set_state(desired=dense['desired'].astype(np.uint16))
    before = take(env)
    flags = _dense_of(before)['flags']
    assert ((flags & ~1) == (2 if style else 0)).all()
    states = dict(dense, flags=flags)                                          # (the engine's states are the oracle's: check_simulate compares the records it read)
    want = oracle_simulate(states, init_grids, acts, stop, RECIPE_KW)
    assert (want['taken'] < T).sum() >= 200 if stop else (want['taken'] == T).all()
    out = _sentinel_out(T, RECIPE_N)
    r = env.simulate(_dev(acts), hdr=env.hdr.clone(), slot_pos=env.slot_pos.clone(), stop_at_done=stop, fields=FIELDS, out=out)
    assert all(r[f] is out[f] for f in FIELDS)
    part, skipped = check_simulate(before, take(env), dict(hdr=before['hdr'], slot_pos=before['slot_pos']), None, acts, stop, _host(out), SENT,
                                   oracle_kw=RECIPE_KW, expected=(states, want))
    assert (part, skipped) == (RECIPE_N, 0)
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 2. against the engine's own step
@pytest.mark.parametrize('mid_episode', [False, True])
def test_against_the_engines_own_step_on_packed_bytes(mid_episode):
    """simulate(stop_at_done=False) first, then the same T steps by step(): hdr / slot_pos byte-equal to the engine's buffers (slot order and flags, which
    decode() does not pin), the traces equal to the rewards / dones the steps returned.  mid_episode: after a spread, with held and vanished slots."""
    T = 12
    env, _, _ = make_env(N1, *np_states(N1, 61000), **ENGINES['state_manual'], **K5)
    env.reset()
    if mid_episode:
        spread(env, 9, 2)
    before = take(env)
    if mid_episode:
        p = before['slot_pos'].view(np.uint16)
        assert (p == POS_HELD).any() and (p == POS_GONE).any() and (before['state_step_num'] > 0).any()      # (held and vanished slots are present)
    acts = _plans(62 + mid_episode, T, N1)
    states = _dense_of(before)
    want = oracle_simulate(dict(states, desired=_near_goals(states, before['state_init_grid'], acts, K5, 3)), before['state_init_grid'], acts, False, K5)
    env.set_state(desired=want['desired'].astype(np.uint16))
    before = take(env)
    paid = want['rewards'] == K5['max_steps']
    if mid_episode:         # 9 steps in, 12 more pass the time-out at 17 unless the spread has just reset the env: time-outs and successes, stepped on past both
        assert (want['dones'] & ~paid).any() and paid.any() and (want['step_num'] > K5['max_steps']).any()
    else:                   # 12 steps from the reset cannot reach the time-out: a done is a success
        assert want['done'].any() and not want['done'].all() and paid.sum() >= 10 and not (want['dones'] & ~paid).any()
    out = _sentinel_out(T, N1)
    t_acts = _dev(acts)
    env.simulate(t_acts, stop_at_done=False, fields=FIELDS, out=out)
    check_simulate(before, take(env), None, None, acts, False, _host(out), SENT, oracle_kw=K5)
    rewards, dones = record_steps(env, t_acts)
    assert torch.equal(env.hdr, out['hdr']) and torch.equal(env.slot_pos, out['slot_pos'])
    got = _host(out)
    same('rewards', 0, got['rewards'].T, rewards.T)
    same('dones', 0, got['dones'].T.astype(bool), dones.T)
    assert np.array_equal(got['ret'], rewards.sum(axis=0)) and np.array_equal(got['achieved_mask'], env.achieved_mask.cpu().numpy())
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 3. against chained expand()
def _chain_states(kind):
    S = 8
    if kind == 'painted':
        _, grid, init, agent, hold = painted_batch(S, 66)
        ach = np.zeros(len(hold), np.int64)
    else:
        grid, init, agent, hold, ach = wall_table(S, [(0, 0), (0, S - 1), (S - 1, 0), (S - 1, S - 1), (0, 4), (4, S - 1)], 1024)
    return S, grid, init, np.asarray(agent), np.asarray(hold), np.asarray(ach)


@pytest.mark.parametrize('kind', ['painted', 'walls'])
def test_against_chained_expand(kind):
    """T = 3 on the painted state classes and on the wall table (the agent in four corners and on two edges): each step picks row [a_t, j] of an expand();
    the final records byte-equal, the rewards and dones equal; with stop_at_done the chain frozen by torch.where"""
    S, grid, init, agent, hold, ach = _chain_states(kind)
    n, T, okw = len(hold), 3, k_of(S)
    env, _, _ = make_env(n, *np_states(n, 63000), obs_mode='state', auto_reset=False, **okw)
    env.reset()
    env.set_state(grid=grid, init_grid=init, agent_rc=agent.astype(np.uint8), init_agent_rc=agent.astype(np.uint8), hold=hold.astype(np.uint8),
                  achieved=ach.astype(np.uint16), step_num=(okw['max_steps'] - 2 - np.arange(n) % 3).astype(np.int32))
    acts = _plans(64, T, n)
    before = take(env)
    env.set_state(desired=_near_goals(_dense_of(before), before['state_init_grid'], acts, okw, 1).astype(np.uint16))
    before = take(env)
    t_acts, cols = _dev(acts), torch.arange(n, device='cuda')
    h, p = env.hdr.clone(), env.slot_pos.clone()
    rew, don = torch.zeros((T, n), dtype=torch.int32, device='cuda'), torch.zeros((T, n), dtype=torch.bool, device='cuda')
    fh, fp, active = h.clone(), p.clone(), torch.ones(n, dtype=torch.bool, device='cuda')       # the chain frozen at a state's first done step
    frew, fdon = rew.clone(), don.clone()
    for t in range(T):
        e = env.expand(hdr=h, slot_pos=p)
        a = t_acts[t].long()
        h, p, rew[t], don[t] = e['hdr'][a, cols], e['slot_pos'][a, cols], e['reward'][a, cols], e['done'][a, cols]
        e = env.expand(hdr=fh, slot_pos=fp)
        fh, fp = torch.where(active[:, None], e['hdr'][a, cols], fh), torch.where(active[:, None], e['slot_pos'][a, cols], fp)
        frew[t], fdon[t] = torch.where(active, e['reward'][a, cols], 0), active & e['done'][a, cols]
        active = active & ~e['done'][a, cols]
    assert don.any() and not don.any(dim=0).all() and (rew == okw['max_steps']).sum() >= 10 and (~active).sum() >= 10 and active.sum() >= 10
    for stop, (wh, wp, wr, wd) in ((False, (h, p, rew, don)), (True, (fh, fp, frew, fdon))):
        out = _sentinel_out(T, n)
        env.simulate(t_acts, stop_at_done=stop, fields=FIELDS, out=out)
        assert torch.equal(out['hdr'], wh) and torch.equal(out['slot_pos'], wp), stop
        assert torch.equal(out['rewards'], wr) and torch.equal(out['dones'], wd) and torch.equal(out['ret'], wr.sum(dim=0).to(torch.int32)), stop
        assert torch.equal(out['done'], wd.any(dim=0)), stop
        check_simulate(before, take(env), None, None, acts, stop, _host(out), SENT, oracle_kw=okw)
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 4. the broadcast form
def _broadcast(engine, S):
    """K = 3 plans for each of 70 envs as actions [T, 3, 70], no records handed in: every engine kind, the frames of the pixel modes untouched"""
    ekw, okw, K, T = dict(ENGINES[engine]), k_of(S), 3, 9
    env, _, _ = make_env(N1, *np_states(N1, 65000), **ekw, **okw)
    env.reset()
    spread(env, 7, 4)
    st = env.get_state()
    sn = st['step_num'].copy()
    sn[::5] = okw['max_steps'] - 3                                # every fifth env three steps before the time-out
    env.set_state(step_num=sn)
    acts = _plans(66, T, K * N1, noops=0.05)
    before = take(env)
    states = _dense_of(before)
    env.set_state(desired=_near_goals(states, before['state_init_grid'], acts[:, :N1], okw, 2).astype(np.uint16))       # (plan 0's goal; plans 1, 2 try others)
    before = take(env)
    tiled = {k: np.tile(v, (K,) + (1,) * (v.ndim - 1)) for k, v in _dense_of(before).items() if k in DENSE}
    want = oracle_simulate(tiled, np.tile(before['state_init_grid'], (K, 1, 1)), acts, True, okw)
    first = want['rewards'][np.minimum(want['length'] - 1, T - 1), np.arange(K * N1)]
    assert (want['done'] & (first == okw['max_steps'])).sum() >= 5 and (want['done'] & (first == -1)).sum() >= 20 and (~want['done']).sum() >= 30
    out = _sentinel_out(T, K * N1)
    r = env.simulate(_dev(acts).reshape(T, K, N1), fields=FIELDS, out=out)
    assert all(r[f] is out[f] for f in FIELDS)
    after = take(env)                                             # (every buffer, stream, frame and counter: check_simulate compares them all)
    if env.obs_mode != 'state':
        assert 'observation' in before and 'desired_goal' in before
    part, _ = check_simulate(before, after, None, None, acts.reshape(T, K, N1), True, _host(out), SENT, oracle_kw=okw, expected=(tiled, want))
    assert part == K * N1
    flat = env.simulate(acts)                                     # the host path, [T, K * N], the default fields
    assert set(flat) == set(FIELDS[:6]) and all(torch.equal(flat[f], out[f]) for f in flat)
    env.close()


@pytest.mark.parametrize('engine', list(ENGINES))
def test_broadcast_form_on_every_engine(engine):
    _broadcast(engine, 5)


@pytest.mark.parametrize('size', [x for x in SIZES if x != 5])
@pytest.mark.parametrize('engine', list(ENGINES))
def test_broadcast_form_on_every_engine_at_size(engine, size):
    _broadcast(engine, size)


def test_broadcast_form_on_a_large_grid():
    """255 x 255, N = 9, T = 5: slot cells above 32 767 (negative in the int16 tensors), rows and columns above 127"""
    S, N, K, T = 255, 9, 2, 5
    okw = k_of(S)
    names, grid, init, agent, hold = painted_batch(S, 22)
    far = [j for j in range(22) if max(agent[j]) >= 128][:N]
    assert len(far) == N
    grid, init, agent, hold = grid[far], init[far], agent[far], hold[far]
    env, _, _ = make_env(N, *np_states(N, 67000), obs_mode='state', auto_reset=False, **okw)
    env.reset()
    env.set_state(grid=grid, init_grid=init, agent_rc=agent, init_agent_rc=agent, hold=hold, step_num=np.full(N, okw['max_steps'] - 4, np.int32))
    before = take(env)
    acts = _plans(68, T, K * N)
    env.set_state(desired=_near_goals(_dense_of(before), before['state_init_grid'], acts[:, :N], okw, 2).astype(np.uint16))
    before = take(env)
    above = int(((before['slot_pos'].view(np.uint16) > 32767) & (before['slot_pos'].view(np.uint16) < POS_HELD)).sum())
    assert above >= N and (before['slot_pos'] < -2).sum() == above
    for stop in (True, False):
        out = _sentinel_out(T, K * N)
        env.simulate(_dev(acts), stop_at_done=stop, fields=FIELDS, out=out)
        part, _ = check_simulate(before, take(env), None, None, acts, stop, _host(out), SENT, oracle_kw=okw)
        assert part == K * N
    assert out['done'].any() and (out['slot_pos'].cpu().numpy() < -2).any()
    env.close()


def test_host_outputs_engine():
    """an engine whose outputs live in mapped host memory: the same call, synchronised on return"""
    env, _, _ = make_env(4, *np_states(4, 69000), obs_mode='pixels_dirty', host_outputs=True, auto_reset=False, **K5)
    env.reset()
    for a in (1, 2, 4, 1, 5, 0):
        env.step(np.full(4, a, np.int32))
    before = take(env)
    acts = _plans(70, 9, 8)
    r = env.simulate(acts, fields=FIELDS)
    check_simulate(before, take(env), None, None, acts, True, _host(r), SENT, oracle_kw=K5)
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 5. launch and loop edges
@pytest.fixture(scope='module')
def engine70():
    env = walked_engine(71000, 6)
    yield env
    env.close()


def _records(before, M, seed, with_env_of=True):
    """M records of the caller's from a 70-env engine: the envs' own with other step counts and menu bytes -> (env_of as records_gpu.env_of_cases draws
    it, or None: record j is env j % 70's; hdr, pos)"""
    if not with_env_of:
        return (None,) + caller_records(before, np.arange(M) % N1, M, N1, K5['max_steps'])
    e = env_of_cases(M, N1) if M >= 63 else np.random.RandomState(seed).randint(0, N1, M).astype(np.int64)
    return (e,) + caller_records(before, e, M, N1, K5['max_steps'])


def _edge_call(env, M, T, stop, seed, fields=FIELDS, with_env_of=True, noops=0.08):
    before = take(env)
    e, hdr, pos = _records(before, M, seed, with_env_of)
    acts = _plans(seed, T, M, noops=noops)
    out = _sentinel_out(T, M, fields)
    skipped0 = env.expand_skipped
    r = env.simulate(_dev(acts), _dev(hdr), _dev(pos, np.int16), None if e is None else _dev(e, np.int32), stop_at_done=stop, fields=fields, out=out)
    assert list(r) == list(fields)
    part, skipped = check_simulate(before, take(env), dict(hdr=hdr, slot_pos=pos), e, acts, stop, _host(out), SENT, oracle_kw=K5)
    assert env.expand_skipped == skipped0 + skipped
    return e, part, skipped, out


@pytest.mark.parametrize('M', [1, 63, 64, 65, 255, 256, 257, 4097])
def test_launch_edges(engine70, M):
    """M states around the wave and the workgroup; from 63 states on env_of mixes valid ids, repeats, -1, -7, N, N + 31 and INT32_MAX: the rows of those
    states, trace rows included, still hold the sentinel, and the skipped ones are counted once each"""
    e, part, skipped, _ = _edge_call(engine70, M, BLOCK + 1, True, 100 + M)
    assert part == int(((e >= 0) & (e < N1)).sum()) and skipped == int((e >= N1).sum())
    if M >= 63:
        assert skipped >= 3 and (e < 0).sum() >= 2
    if M == 4097:
        assert skipped >= 6 and part >= 4000
        with pytest.raises(IndexError):                                            # the host-validated path refuses what the kernel skips
            engine70.simulate(_plans(1, 2, M), np.zeros((M, 16), np.uint8), np.zeros((M, 8), np.int16), e)


@pytest.mark.parametrize('stop', [True, False])
@pytest.mark.parametrize('T', [1, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1])
def test_horizons_around_the_action_block(engine70, T, stop):
    """T = 1, 7, 8, 9, 17: below, at and above one block of prefetched action bytes, and two blocks and one; action ids 6, 200 and 255 mixed in"""
    _edge_call(engine70, 65, T, stop, 200 + T, with_env_of=False, noops=0.15)


def test_stepping_on_past_the_time_out(engine70):
    """T = 40 > max_steps = 17 with stop_at_done=False: every state runs into the time-out and steps on, satisfied goals pay again"""
    env, T = engine70, 40
    before = take(env)
    acts = _plans(301, T, 2 * N1)
    states = _dense_of(before)
    near = _near_goals(states, before['state_init_grid'], acts[:, :N1], K5, 2)
    env.set_state(desired=near.astype(np.uint16))
    before = take(env)
    tiled = {k: np.tile(v, (2,) + (1,) * (v.ndim - 1)) for k, v in _dense_of(before).items() if k in DENSE}
    want = oracle_simulate(tiled, np.tile(before['state_init_grid'], (2, 1, 1)), acts, False, K5)
    behind = np.arange(T)[:, None] >= want['length'][None, :]
    assert want['done'].all() and (want['step_num'] > K5['max_steps']).all() and ((want['rewards'] == K5['max_steps']) & behind).sum() >= 10
    assert (want['flags'] >> 2).max() >= 2                                      # (the success count of a record: several successes in one run)
    out = _sentinel_out(T, 2 * N1)
    env.simulate(_dev(acts), stop_at_done=False, fields=FIELDS, out=out)
    check_simulate(before, take(env), None, None, acts, False, _host(out), SENT, oracle_kw=K5, expected=(tiled, want))


def test_a_wave_whose_states_have_all_ended(engine70):
    """64 states that all end within two steps while T = 17, beside a wave of states that do not: the first wave leaves the step loop and must still write
    the reward-0 / done-0 rows that remain -- not leave the sentinel there"""
    env, T, C0 = engine70, 2 * BLOCK + 1, 16 * N1
    before = take(env)
    src = np.arange(C0) % N1
    acts = _plans(302, T, C0)
    cand = {k: v[src] for k, v in _dense_of(before).items() if k in DENSE}
    cand['step_num'] = np.minimum(cand['step_num'], 5)
    cand['desired'] = oracle_simulate(cand, before['state_init_grid'][src], acts[:1], False, K5)['achieved']       # desired := the achieved mask after one step
    want = oracle_simulate(cand, before['state_init_grid'][src], acts, True, K5)
    early, late = np.flatnonzero(want['length'] <= 2), np.flatnonzero(want['length'] > 2)
    assert len(early) >= 64 and len(late) >= 64
    pick = np.concatenate([early[:64], late[:64]])
    hdr, pos = before['hdr'][src[pick]].copy(), before['slot_pos'][src[pick]].copy()
    hdr[:, 6], hdr[:, 7] = cand['desired'][pick] & 0xFF, cand['desired'][pick] >> 8
    hdr[:, 8], hdr[:, 9] = cand['step_num'][pick], 0
    acts = np.ascontiguousarray(acts[:, pick])
    for fields in (FIELDS, TRACES):
        out = _sentinel_out(T, 128, fields)
        env.simulate(_dev(acts), _dev(hdr), _dev(pos, np.int16), _dev(src[pick], np.int32), fields=fields, out=out)
        got = _host(out)
        check_simulate(before, take(env), dict(hdr=hdr, slot_pos=pos), src[pick], acts, True, got, SENT, oracle_kw=K5)
        assert (got['rewards'][2:, :64] == 0).all() and (got['dones'][2:, :64] == 0).all() and got['dones'][:2, :64].sum() == 64


@pytest.mark.parametrize('fields', [('ret',), ('rewards',), ('hdr', 'slot_pos'), ('dones', 'length'), ('slot_pos',), ('hdr',)])
def test_subsets_of_the_fields(engine70, fields):
    _, part, _, out = _edge_call(engine70, 65, BLOCK + 1, True, 400, fields=fields)
    assert set(out) == set(fields) and part > 50


def test_no_states(engine70):
    env = engine70
    r = env.simulate(torch.empty((5, 0), dtype=torch.uint8, device='cuda'), hdr=torch.empty((0, 16), dtype=torch.uint8, device='cuda'),
                     slot_pos=torch.empty((0, 8), dtype=torch.int16, device='cuda'), fields=FIELDS)
    assert set(r) == set(FIELDS) and tuple(r['rewards'].shape) == (5, 0) and tuple(r['hdr'].shape) == (0, 16)


# ------------------------------------------------------------------------------------------------------------------------------ 6. errors
def test_bad_arguments_of_the_method(engine70):
    env = engine70
    acts = _dev(_plans(5, 4, N1))
    good = env.simulate(acts, fields=FIELDS)
    h, p = env.hdr.clone(), env.slot_pos.clone()
    own = env.simulate(acts, h, p, fields=FIELDS)
    assert all(torch.equal(own[f], good[f]) for f in FIELDS)
    big_h, big_p = torch.zeros((N1 + 1, 16), dtype=torch.uint8, device='cuda'), torch.zeros((N1 + 1, 8), dtype=torch.int16, device='cuda')
    odd = torch.zeros(16 * N1 + 16, dtype=torch.uint8, device='cuda')[8:8 + 16 * N1].view(N1, 16)
    assert odd.is_contiguous() and odd.data_ptr() % 16 == 8
    for bad in (dict(fields=[]), dict(fields=['ret', 'frames']), dict(fields=['done', 'done']), dict(hdr=h), dict(slot_pos=p),
                dict(env_of=torch.zeros(N1, dtype=torch.int32, device='cuda')), dict(actions=acts[:, :N1 - 1]), dict(actions=acts[:0]),
                dict(actions=acts.to(torch.float32)), dict(actions=acts.cpu().numpy().astype(np.int64) + 251), dict(actions=-acts.cpu().numpy().astype(np.int64) - 1),
                dict(actions=torch.zeros((32768, N1), dtype=torch.uint8, device='cuda')), dict(actions=acts.reshape(4, 1, 1, N1)),
                dict(hdr=h[:5], slot_pos=p), dict(hdr=h[:5], slot_pos=p[:5]), dict(out={'ret': good['ret']}),
                dict(out=dict(good, ret=good['ret'].to(torch.int64))), dict(out=dict(good, rewards=good['rewards'][:3])), dict(out=dict(good, done=good['done'].cpu())),
                dict(hdr=h, slot_pos=p, out=dict(good, hdr=h)), dict(hdr=h, slot_pos=p, out=dict(good, slot_pos=p)),       # the output IS the input
                dict(hdr=h, slot_pos=p, out=dict(good, hdr=p.view(torch.uint8))),                                          # ... is the other input
                dict(hdr=big_h[:-1], slot_pos=big_p[:-1], out=dict(good, hdr=big_h[1:])),                                  # ... overlaps it by all rows but one
                dict(hdr=big_h[:-1], slot_pos=big_p[:-1], out=dict(good, slot_pos=big_p[1:])),
                dict(out=dict(good, hdr=env.hdr)), dict(out=dict(good, slot_pos=env.slot_pos)),                             # the broadcast form reads the engine's own
                dict(hdr=odd, slot_pos=p), dict(out=dict(good, hdr=odd))):                                                 # not 16-byte aligned
        kw = dict(dict(actions=acts, fields=FIELDS), **bad)
        with pytest.raises(ValueError):
            env.simulate(kw.pop('actions'), **kw)
    with pytest.raises(IndexError):
        env.simulate(acts.cpu().numpy(), h.cpu().numpy(), p.cpu().numpy(), np.arange(N1) + 1)
    assert torch.equal(env.simulate(acts, fields=['ret'])['ret'], good['ret'])


def test_call_order_and_arguments_through_ctypes():
    from gym_craftingworld_amd import CraftingWorldVecEnv, _lib as L
    N, T = 8, 3
    env = CraftingWorldVecEnv(N, obs_mode='state', auto_reset=False, seed=3, **K5)
    lib, h, st = env._lib, env._h, env._stream()
    bufs = _sentinel_out(T, N)
    acts = _dev(_plans(6, T, N))
    vp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    one = lambda **kw: L.cw_simulate_out(**kw)  # noqa: E731
    full = one(ret=vp(bufs['ret']), length=vp(bufs['length']), done=vp(bufs['done']), achieved=vp(bufs['achieved_mask']), hdr=vp(bufs['hdr']),
               slot_pos=vp(bufs['slot_pos']), rewards=vp(bufs['rewards']), dones=vp(bufs['dones']))
    with pytest.raises(L.CraftingWorldError):                                      # before reset(), through the method
        env.simulate(acts)
    assert lib.cw_simulate(h, None, None, None, N, vp(acts), T, 1, C.byref(full), st) == L.CW_ERR_STATE and b'before cw_reset' in lib.cw_last_error()
    env.reset()
    hdr, pos, eo = vp(env.hdr), vp(env.slot_pos), vp(torch.zeros(N, dtype=torch.int32, device='cuda'))
    ch, cp = env.hdr.clone(), env.slot_pos.clone()
    assert lib.cw_simulate(h, None, None, None, N, vp(acts), T, 1, C.byref(full), st) == L.CW_OK
    assert lib.cw_simulate(h, None, vp(ch), vp(cp), 0, vp(acts), T, 1, C.byref(full), st) == L.CW_OK       # no states: nothing enqueued
    a = vp(acts)
    invalid = [((None, None, None, None, N, a, T, 1, C.byref(full)), b'engine'),
               ((h, None, None, None, N, a, T, 1, None), b'out'),
               ((h, None, None, None, N, None, T, 1, C.byref(full)), b'actions'),
               ((h, None, None, None, N, a, T, 1, C.byref(one())), b'every field'),
               ((h, None, vp(ch), vp(cp), -1, a, T, 1, C.byref(full)), b'n_states'),
               ((h, None, vp(ch), vp(cp), 2 ** 27 + 1, a, T, 1, C.byref(full)), b'n_states'),
               ((h, None, None, None, N, a, 0, 1, C.byref(full)), b'n_steps'),
               ((h, None, None, None, N, a, 32768, 1, C.byref(full)), b'n_steps'),
               ((h, None, None, None, N - 1, a, T, 1, C.byref(full)), b'multiple of num_envs'),
               ((h, None, None, None, 0, a, T, 1, C.byref(full)), b'multiple of num_envs'),
               ((h, None, vp(ch), None, N, a, T, 1, C.byref(full)), b'hdr_in given without slot_pos_in'),
               ((h, None, None, vp(cp), N, a, T, 1, C.byref(full)), b'slot_pos_in given without hdr_in'),
               ((h, eo, None, None, N, a, T, 1, C.byref(full)), b'env_of'),
               ((h, None, vp(ch, 8), vp(cp), N - 1, a, T, 1, C.byref(full)), b'hdr_in is not 16-byte aligned'),
               ((h, None, vp(ch), vp(cp, 2), N - 1, a, T, 1, C.byref(full)), b'slot_pos_in is not 16-byte aligned'),
               ((h, None, vp(ch), vp(cp), N - 1, a, T, 1, C.byref(one(hdr=vp(bufs['hdr'], 4)))), b'out->hdr is not 16-byte aligned'),
               ((h, None, vp(ch), vp(cp), N - 1, a, T, 1, C.byref(one(ret=vp(bufs['ret']), slot_pos=vp(bufs['slot_pos'], 8)))), b'out->slot_pos is not 16-byte aligned'),
               ((h, None, vp(ch), vp(cp), N, a, T, 1, C.byref(one(hdr=vp(ch)))), b'out->hdr overlaps'),
               ((h, None, vp(ch), vp(cp), N - 1, a, T, 1, C.byref(one(slot_pos=vp(cp, 16 * (N - 2))))), b'out->slot_pos overlaps'),
               ((h, None, None, None, N, a, T, 1, C.byref(one(hdr=hdr))), b'out->hdr overlaps'),
               ((h, None, None, None, 2 * N, a, T, 1, C.byref(one(slot_pos=pos))), b'out->slot_pos overlaps')]
    for args, word in invalid:
        assert lib.cw_simulate(*args, st) == L.CW_ERR_INVALID, word
        assert word in lib.cw_last_error(), (word, lib.cw_last_error())
    torch.cuda.synchronize()
    assert env.expand_skipped == 0
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 7. capture
def test_captured_into_a_graph():
    """torch.cuda.graph around one simulate(out=...): the call only enqueues; replayed after the env has stepped and the action tensor was refilled in
    place it equals an eager simulate() of the new state and plans"""
    N, K, T = 300, 2, BLOCK + 1
    env, _, _ = make_env(N, *np_states(N, 72000), obs_mode='state', **K5)
    env.reset()
    spread(env, 5, 6)
    acts = _dev(_plans(7, T, K * N))
    out = _sentinel_out(T, K * N)
    env.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.simulate(acts, fields=FIELDS, out=out)
    assert all(bool((t.view(torch.uint8) == SENT).all()) for t in out.values())          # (capturing ran nothing)
    for rnd in range(3):
        spread(env, 3, 7 + rnd)
        acts.copy_(_dev(_plans(8 + rnd, T, K * N, noops=0.05)))
        g.replay()
        eager = env.simulate(acts, fields=FIELDS)
        for f in FIELDS:
            assert torch.equal(out[f], eager[f]), (rnd, f)
    before = take(env)
    g.replay()
    torch.cuda.synchronize()
    check_simulate(before, take(env), None, None, acts.cpu().numpy(), True, _host(out), SENT, oracle_kw=K5)
    env.close()
