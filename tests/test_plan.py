"""GPU tier of searching every plan: cw_plan_kernel through CraftingWorldVecEnv.plan.  The shared recipe is checked row by row with plan_check.check_plan
(itself tested on the CPU, tests/test_plan_logic.py) against the CPU oracle's enumeration of all 6^D strings; the deep levels, which the oracle cannot
enumerate, against simulate() of all 6^D strings on the device, reduced by the rule of craftingworld.h with torch; depth 1 against expand(); the plans fed
back through simulate(); the engine before and after every checked call byte for byte.  Everything is bit-exact.  No timing."""
import numpy as np
import pytest
import torch

from engines import ENGINES, K5, N1, k_of
from masked_check import spread, take
from oracle_replay import make_env, np_states
from plan_check import FIELDS, RECIPE_KW, RECIPE_N, RECIPE_PART, assert_recipe_coverage, check_plan, coverage, layout, recipe, recipe_plans
from records_check import POS_HELD, encode
from records_gpu import SENT, caller_records, dev as _dev, env_of_cases as _env_of, host, sentinel_out, walk_goals as _walk_goals, walked_engine
from state_tables import painted_batch, wall_table

pytestmark = pytest.mark.gpu

_WIDTH = dict(q=4, length=4, done=1, achieved_mask=2, hdr=16, slot_pos=16, plan=1)
_DTYPE = dict(q=torch.int32, length=torch.int32, done=torch.bool, achieved_mask=torch.int16, hdr=torch.uint8, slot_pos=torch.int16, plan=torch.uint8)
PER_PLAN = ('length', 'done', 'achieved_mask', 'hdr', 'slot_pos')      # what simulate() returns for a plan besides its return


def _sentinel_out(D, M):
    """output buffers as plan(out=...) takes them, every byte SENT"""
    return sentinel_out(layout(D), _WIDTH, _DTYPE, M)


def _host(r):
    return host(r, FIELDS)


def _enumerated(env, D, hdr, pos, env_of=None):
    """the same results the long way round, on the device: simulate(stop_at_done=True) of all 6^D strings of every record, reduced by the rule of
    craftingworld.h -- the maximum over the strings that begin with a, the smallest string that reaches it (no argmax, whose ties are not pinned), its
    digits behind its end zeroed -> the seven fields"""
    M, n = hdr.shape[0], 6 ** D
    s = torch.arange(n, device='cuda')
    digits = torch.stack([(s // 6 ** (D - 1 - t)) % 6 for t in range(D)]).to(torch.uint8)                 # [D, 6^D]
    acts = digits[:, :, None].expand(D, n, M).reshape(D, n * M).contiguous()                               # column s * M + j: string s of record j
    eo = (torch.arange(M, device='cuda', dtype=torch.int32) % env.num_envs) if env_of is None else env_of
    r = env.simulate(acts, hdr.repeat(n, 1), pos.repeat(n, 1), eo.repeat(n))
    ret = r['ret'].view(6, n // 6, M)
    q = ret.amax(dim=1)
    first = torch.where(ret == q[:, None, :], torch.arange(n // 6, device='cuda')[None, :, None], n).amin(dim=1) + torch.arange(6, device='cuda')[:, None] * (n // 6)
    flat = first * M + torch.arange(M, device='cuda')[None, :]
    out = {f: r[f][flat] for f in PER_PLAN}
    out['q'] = q
    plan = torch.stack([(first // 6 ** (D - 1 - t)) % 6 for t in range(D)], dim=1)
    out['plan'] = torch.where(torch.arange(D, device='cuda')[None, :, None] < out['length'][:, None, :], plan, 0).to(torch.uint8)
    return out


# ------------------------------------------------------------------------------------------------------------------------------ 1. the shared recipe
@pytest.fixture(scope='module')
def recipe_coverage():
    """what the recipe exercises under each reward rule, counted from the oracle alone and asserted before anything is compared"""
    cov = {}
    for style in (None, 'subset'):
        cov[style] = {D: coverage(recipe_plans(D, style)[1], D) for D in range(1, 6)}
        assert_recipe_coverage(cov[style])
    return cov


@pytest.mark.parametrize('style', [None, 'subset'])
@pytest.mark.parametrize('D', [1, 2, 3, 4, 5])
def test_the_recipe_against_the_oracle(recipe_coverage, D, style):
    """600 records -- two full workgroups and a 24-lane tail wave -- handed in through hdr= / slot_pos= / env_of=; 600, 100 or 24 of them take part
    (plan_check.recipe), the rest hold -1 and their rows the sentinel; all seven fields into sentinel-filled buffers, under both reward rules"""
    dense, init_grids, env_of = recipe(D, style)
    env, _, _ = make_env(RECIPE_N, *np_states(RECIPE_N, 900), obs_mode='state', reward_style=style, auto_reset=False, **RECIPE_KW)
    env.reset()
    before = take(env)
    assert np.array_equal(before['state_init_grid'], init_grids)                  # (env j's episode is oracle env j's: it supplies the start positions)
    hdr, pos = encode(dense, menu=before['hdr'][:, 3])
    out = _sentinel_out(D, RECIPE_N)
    r = env.plan(D, _dev(hdr), _dev(pos.view(np.int16), np.int16), _dev(env_of, np.int32), fields=FIELDS, out=out)
    assert all(r[f] is out[f] for f in FIELDS)
    part, skipped = check_plan(before, take(env), dict(hdr=hdr, slot_pos=pos), env_of, D, _host(out), SENT, oracle_kw=RECIPE_KW, expected=recipe_plans(D, style))
    assert (part, skipped) == (RECIPE_PART[D], 0)
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 2. depth 1 is expand()
def _table(kind, S):
    if kind == 'painted':
        _, grid, init, agent, hold = painted_batch(S, 66)
        ach = np.zeros(len(hold), np.int64)
    else:
        grid, init, agent, hold, ach = wall_table(S, [(0, 0), (0, S - 1), (S - 1, 0), (S - 1, S - 1), (0, S // 2), (S // 2, S - 1)], 1024)
    return grid, init, np.asarray(agent), np.asarray(hold), np.asarray(ach)


@pytest.mark.parametrize('kind,S', [('walked', 4), ('painted', 8), ('walls', 8), ('painted', 21), ('walls', 21)])
def test_depth_one_is_expand(kind, S):
    """plan(1) against expand() byte for byte on the painted state classes and the wall table (4 x 4 is below what the tables are built for: there 300 envs
    nine random steps into their episodes): q == reward, done, achieved_mask, hdr, slot_pos, length 1, plan[a, 0] == a; every third state one step before
    its time-out, every other goal the mask one random step reaches"""
    okw = k_of(S)
    if kind == 'walked':
        n = 300
        env, _, _ = make_env(n, *np_states(n, 81000), obs_mode='state', auto_reset=False, **okw)
        env.reset()
        spread(env, 9, 5)
        env.set_state(step_num=(okw['max_steps'] - 1 - np.arange(n) % 3).astype(np.int32))
    else:
        grid, init, agent, hold, ach = _table(kind, S)
        n = len(hold)
        env, _, _ = make_env(n, *np_states(n, 81000), obs_mode='state', auto_reset=False, **okw)
        env.reset()
        env.set_state(grid=grid, init_grid=init, agent_rc=agent.astype(np.uint8), init_agent_rc=agent.astype(np.uint8), hold=hold.astype(np.uint8),
                      achieved=ach.astype(np.uint16), step_num=(okw['max_steps'] - 1 - np.arange(n) % 3).astype(np.int32))
    _walk_goals(env, 1, 82)
    e = env.expand()
    assert e['done'].any() and not e['done'].all() and (e['reward'] == okw['max_steps']).sum() >= 10 and (e['reward'] == -1).sum() >= 10
    out = _sentinel_out(1, n)
    env.plan(1, fields=FIELDS, out=out)
    assert torch.equal(out['q'], e['reward']) and torch.equal(out['done'], e['done']) and torch.equal(out['achieved_mask'], e['achieved_mask'])
    assert torch.equal(out['hdr'], e['hdr']) and torch.equal(out['slot_pos'], e['slot_pos']) and bool((out['length'] == 1).all())
    assert torch.equal(out['plan'][:, 0], torch.arange(6, dtype=torch.uint8, device='cuda')[:, None].expand(6, n))
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 3. the deep levels
@pytest.fixture(scope='module')
def deep_states():
    """a 70-env engine mid-episode; records 0..3 of the deep test: 0 and 2 with a goal a 3-step walk reaches, 1 three steps from its time-out, 3 as it is"""
    env, _, _ = make_env(N1, *np_states(N1, 83000), obs_mode='state', auto_reset=False, **K5)
    env.reset()
    spread(env, 9, 2)
    _walk_goals(env, 3, 84)
    sn = env.get_state()['step_num'].copy()
    sn[0], sn[2], sn[3] = 2, 3, 1
    sn[1] = K5['max_steps'] - 3
    env.set_state(step_num=sn)
    yield env
    env.close()


@pytest.mark.parametrize('D', [6, 7, 8])
def test_deep_levels_against_simulate(deep_states, D):
    """levels 6, 7 and 8 of the register stack: 4 records, all 6^D strings of each (6.7 M states at D = 8) through simulate(), itself oracle-tested; every
    field of every (first action, record) pair"""
    env = deep_states
    hdr, pos = env.hdr[:4].clone(), env.slot_pos[:4].clone()
    want = _enumerated(env, D, hdr, pos)
    ok = want['done'] & (want['q'] > 0)
    assert ok[:, 0].any() and ok[:, 2].any() and bool((want['length'][:, 1] <= 3).all()) and bool(want['done'][:, 1].all())        # two goals within reach, one time-out
    assert bool((want['q'][:, 1][~ok[:, 1]] == -3).all())
    before = take(env)
    out = _sentinel_out(D, 4)
    env.plan(D, hdr, pos, fields=FIELDS, out=out)
    for f in FIELDS:
        assert torch.equal(out[f], want[f]), (D, f)
    after = take(env)
    assert all(np.array_equal(before[k], after[k]) for k in before)
    best = env.plan(D, hdr, pos, fields=('q', 'best_action', 'best_q'))
    q = want['q'].cpu().numpy()
    assert np.array_equal(best['best_q'].cpu().numpy(), q.max(axis=0)) and best['best_action'].dtype == torch.uint8
    assert best['best_action'].tolist() == [min(a for a in range(6) if q[a, j] == q[:, j].max()) for j in range(4)]


@pytest.mark.parametrize('D', [2, 3, 4, 5])
def test_shallow_levels_against_simulate_on_many_states(deep_states, D):
    """the same comparison at the depths the oracle also covers, on all 70 envs' own states (no records handed in): the two references agree with the
    kernel and so with each other"""
    env = deep_states
    want = _enumerated(env, D, env.hdr.clone(), env.slot_pos.clone())
    got = env.plan(D, fields=FIELDS)
    for f in FIELDS:
        assert torch.equal(got[f], want[f]), (D, f)
    assert (want['done'] & (want['q'] > 0)).sum() >= 20 and (~want['done']).sum() >= 20


# ------------------------------------------------------------------------------------------------------------------------------ 4. closing the loop
@pytest.mark.parametrize('D', [1, 4, 6])
def test_the_plans_fed_back_through_simulate(deep_states, D):
    """plan[a] IS an action tensor of simulate(): stepping it with stop_at_done=True reproduces q, length, done, achieved_mask, hdr and slot_pos of row a,
    byte for byte, for all six first actions"""
    env = deep_states
    M = N1 if D < 6 else 8
    hdr, pos = env.hdr[:M].clone(), env.slot_pos[:M].clone()
    got = env.plan(D, hdr, pos, fields=FIELDS)
    assert got['done'].any() and not got['done'].all() and (got['length'] < D).any() == (D > 1)
    for a in range(6):
        assert bool((got['plan'][a, 0] == a).all())
        r = env.simulate(got['plan'][a], hdr, pos, stop_at_done=True)
        assert torch.equal(r['ret'], got['q'][a]), a
        for f in PER_PLAN:
            assert torch.equal(r[f], got[f][a]), (a, f)


def test_following_best_action_reaches_the_goal_on_the_planned_step():
    """the receding-horizon controller on an auto_reset=False engine: plan(D), step(best_action), again.  An env whose best plan ends by success at
    length L is paid max_steps on exactly its L-th step, and -1 on every step before"""
    D, N = 4, 300
    env, _, _ = make_env(N, *np_states(N, 85000), obs_mode='state', auto_reset=False, **K5)
    env.reset()
    spread(env, 4, 3)
    env.set_state(step_num=np.full(N, 2, np.int32))
    _walk_goals(env, 4, 86, every=1)
    first = env.plan(D)
    assert set(first) == {'q', 'length', 'done', 'achieved_mask', 'plan', 'best_action', 'best_q'}               # (the default fields)
    a0 = first['best_action'].long()
    cols = torch.arange(N, device='cuda')
    L = first['length'][a0, cols]
    wins = first['done'][a0, cols] & (first['best_q'] == K5['max_steps'] + 1 - L)
    assert int(wins.sum()) >= 50 and int((wins & (L == 1)).sum()) >= 5 and int((wins & (L >= 2)).sum()) >= 5, (int(wins.sum()), L[wins].tolist())
    rewards = torch.empty((D, N), dtype=torch.int32, device='cuda')
    best = first
    for t in range(D):
        _, rew, _, _ = env.step(best['best_action'])
        rewards[t] = rew
        best = env.plan(D, fields=('best_action', 'best_q'))
    t = torch.arange(D, device='cuda')[:, None]
    want = torch.where(t == (L - 1)[None, :], K5['max_steps'], -1).to(torch.int32)
    planned = (t < L[None, :]) & wins[None, :]                                    # the steps of the plans that win, up to their last
    assert torch.equal(rewards[planned], want[planned]) and int((rewards[planned] == K5['max_steps']).sum()) == int(wins.sum())
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 5. env_of
@pytest.fixture(scope='module')
def engine70():
    env = walked_engine(87000, 9, goals=(2, 88))
    yield env
    env.close()


def _records(before, e, M):
    return caller_records(before, e, M, N1, K5['max_steps'])


@pytest.mark.parametrize('M,D', [(63, 3), (65, 2), (257, 2), (1000, 1)])
def test_env_of_on_the_device(engine70, M, D):
    """env_of handed over as a device tensor: random envs with repeats, -1 and -7 (no part: sentinel rows in all seven fields), N, N + 31 and INT32_MAX
    (skipped, and counted once each -- not once per first action)"""
    env = engine70
    e = _env_of(M, N1)
    before = take(env)
    hdr, pos = _records(before, e, M)
    out = _sentinel_out(D, M)
    skipped0 = env.expand_skipped
    env.plan(D, _dev(hdr), _dev(pos, np.int16), _dev(e, np.int32), fields=FIELDS, out=out)
    part, skipped = check_plan(before, take(env), dict(hdr=hdr, slot_pos=pos), e, D, _host(out), SENT, oracle_kw=K5)
    assert skipped == int((e >= N1).sum()) >= 2 and part == int(((e >= 0) & (e < N1)).sum()) and (e < 0).sum() >= 2
    assert env.expand_skipped == skipped0 + skipped
    with pytest.raises(IndexError):                                               # the host-validated path refuses what the kernel skips
        env.plan(D, hdr, pos, e)
    if M == 65:                                                                   # every single field: the other buffers stay as they were
        for f in FIELDS:
            bufs = _sentinel_out(D, M)
            before = take(env)
            r = env.plan(D, _dev(hdr), _dev(pos, np.int16), _dev(e, np.int32), fields=[f], out={f: bufs[f]})
            assert list(r) == [f]
            check_plan(before, take(env), dict(hdr=hdr, slot_pos=pos), e, D, _host(r), SENT, oracle_kw=K5)
            assert all(bool((bufs[g].view(torch.uint8) == SENT).all()) for g in FIELDS if g != f), f


def test_a_permutation_uses_each_states_own_start_positions():
    """record j is env perm[j]'s state: the Move tasks of what it holds are judged against THAT env's start positions -- 300 envs that have walked and
    tried to pick up four times, so that many hold something"""
    N, D = 300, 2
    env, _, _ = make_env(N, *np_states(N, 97000), obs_mode='state', auto_reset=False, **K5)
    env.reset()
    for k in range(4):
        spread(env, 2, 10 + k, moves_only=True)
        env.step(torch.full((N,), 4, dtype=torch.uint8, device='cuda'))
        env.reset_envs(env.done)
    _walk_goals(env, 2, 98)
    before = take(env)
    perm = np.random.RandomState(9).permutation(N)
    held = (before['slot_pos'].view(np.uint16) == POS_HELD).any(axis=1)
    assert held.sum() >= 30 and (perm != np.arange(N)).sum() >= 290, int(held.sum())
    hdr, pos = before['hdr'][perm].copy(), before['slot_pos'][perm].copy()
    out = _sentinel_out(D, N)
    env.plan(D, _dev(hdr), _dev(pos, np.int16), _dev(perm, np.int32), fields=FIELDS, out=out)
    part, skipped = check_plan(before, take(env), dict(hdr=hdr, slot_pos=pos), perm, D, _host(out), SENT, oracle_kw=K5)
    assert (part, skipped) == (N, 0)
    own = env.plan(D, fields=FIELDS)                                              # ... and equals the envs' own plans, permuted
    idx = torch.as_tensor(perm, device='cuda')
    for f in FIELDS:
        assert torch.equal(out[f], own[f][:, :, idx] if f == 'plan' else own[f][:, idx]), f
    env.close()


def test_on_a_large_grid():
    """255 x 255, N = 9, D = 2: slot cells above 32 767 (negative in the int16 tensors), rows and columns above 127"""
    S, N, D = 255, 9, 2
    okw = k_of(S)
    names, grid, init, agent, hold = painted_batch(S, 22)
    far = [j for j in range(22) if max(agent[j]) >= 128][:N]
    assert len(far) == N
    grid, init, agent, hold = grid[far], init[far], agent[far], hold[far]
    env, _, _ = make_env(N, *np_states(N, 89000), obs_mode='state', auto_reset=False, **okw)
    env.reset()
    env.set_state(grid=grid, init_grid=init, agent_rc=agent, init_agent_rc=agent, hold=hold, step_num=np.full(N, okw['max_steps'] - 4, np.int32))
    _walk_goals(env, 2, 90)
    sn = env.get_state()['step_num'].copy()
    sn[::3] = okw['max_steps'] - 1
    env.set_state(step_num=sn)
    before = take(env)
    above = int(((before['slot_pos'].view(np.uint16) > 32767) & (before['slot_pos'].view(np.uint16) < POS_HELD)).sum())
    assert above >= N and (before['slot_pos'] < -2).sum() == above
    out = _sentinel_out(D, N)
    env.plan(D, fields=FIELDS, out=out)
    part, _ = check_plan(before, take(env), None, None, D, _host(out), SENT, oracle_kw=okw)
    assert part == N and out['done'].any() and (out['slot_pos'].cpu().numpy() < -2).any()
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 6. every engine kind
def _own_states(ekw, N, seed):
    env, _, _ = make_env(N, *np_states(N, seed), **ekw, **K5)
    env.reset()
    spread(env, 7, 4)
    _walk_goals(env, 2, seed + 1)
    sn = env.get_state()['step_num'].copy()
    sn[::5] = K5['max_steps'] - 2                                 # every fifth env two steps before the time-out
    env.set_state(step_num=sn)
    before = take(env)
    if env.obs_mode != 'state':
        assert 'observation' in before and 'desired_goal' in before
    r = env.plan(3, fields=FIELDS)
    part, skipped = check_plan(before, take(env), None, None, 3, _host(r), SENT, oracle_kw=K5)       # (every buffer, stream, frame and counter: purity)
    assert (part, skipped) == (N, 0)
    assert r['done'].any() and not r['done'].all()
    env.close()


@pytest.mark.parametrize('engine', list(ENGINES))
def test_the_engines_own_states_on_every_engine(engine):
    _own_states(dict(ENGINES[engine]), N1, 91000)


def test_host_outputs_engine():
    """an engine whose outputs live in mapped host memory: the same call, synchronised on return"""
    _own_states(dict(obs_mode='pixels_dirty', host_outputs=True, auto_reset=False), 4, 92000)


def test_no_states_and_bad_arguments_of_the_method(engine70):
    env = engine70
    r = env.plan(5, hdr=torch.empty((0, 16), dtype=torch.uint8, device='cuda'), slot_pos=torch.empty((0, 8), dtype=torch.int16, device='cuda'), fields=FIELDS)
    assert set(r) == set(FIELDS) and tuple(r['plan'].shape) == (6, 5, 0) and tuple(r['hdr'].shape) == (6, 0, 16)
    good = env.plan(2, fields=FIELDS)
    odd = torch.zeros(16 * N1 + 16, dtype=torch.uint8, device='cuda')[8:8 + 16 * N1].view(N1, 16)
    for bad in (dict(depth=0), dict(depth=9), dict(depth=2.0), dict(fields=[]), dict(fields=['q', 'frames']), dict(fields=['done', 'done']), dict(hdr=env.hdr),
                dict(slot_pos=env.slot_pos), dict(env_of=torch.zeros(N1, dtype=torch.int32, device='cuda')), dict(out={'q': good['q']}),
                dict(out=dict(good, q=good['q'].to(torch.int64))), dict(out=dict(good, plan=good['plan'][:, :1])), dict(out=dict(good, done=good['done'].cpu())),
                dict(hdr=env.hdr[:5], slot_pos=env.slot_pos), dict(hdr=odd, slot_pos=env.slot_pos), dict(depth=3, out=good)):
        kw = dict(dict(depth=2, fields=FIELDS), **bad)
        with pytest.raises(ValueError):
            env.plan(kw.pop('depth'), **kw)


def test_errors_of_the_entry_point():
    import ctypes as C
    from gym_craftingworld_amd import CraftingWorldVecEnv, _lib as L
    N, D = 8, 3
    env = CraftingWorldVecEnv(N, obs_mode='state', auto_reset=False, seed=3, **K5)
    lib, h, st = env._lib, env._h, env._stream()
    bufs = _sentinel_out(D, N)
    vp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    one = lambda **kw: L.cw_plan_out(**kw)  # noqa: E731
    full = one(q=vp(bufs['q']), length=vp(bufs['length']), done=vp(bufs['done']), achieved=vp(bufs['achieved_mask']), hdr=vp(bufs['hdr']),
               slot_pos=vp(bufs['slot_pos']), plan=vp(bufs['plan']))
    with pytest.raises(L.CraftingWorldError):                                      # before reset(), through the method
        env.plan(D)
    assert lib.cw_plan(h, None, None, None, N, D, C.byref(full), st) == L.CW_ERR_STATE and b'before cw_reset' in lib.cw_last_error()
    env.reset()
    ch, cp, eo = env.hdr.clone(), env.slot_pos.clone(), vp(torch.zeros(N, dtype=torch.int32, device='cuda'))
    assert lib.cw_plan(h, None, None, None, N, D, C.byref(full), st) == L.CW_OK
    assert lib.cw_plan(h, None, vp(ch), vp(cp), 0, D, C.byref(full), st) == L.CW_OK                 # no states: nothing enqueued
    invalid = [((None, None, None, None, N, D, C.byref(full)), b'engine'),
               ((h, None, None, None, N, D, None), b'out'),
               ((h, None, None, None, N, D, C.byref(one())), b'every field'),
               ((h, None, vp(ch), vp(cp), -1, D, C.byref(full)), b'n_states'),
               ((h, None, vp(ch), vp(cp), 2 ** 27 + 1, D, C.byref(full)), b'n_states'),
               ((h, None, None, None, N, 0, C.byref(full)), b'depth'),
               ((h, None, None, None, N, 9, C.byref(full)), b'depth'),
               ((h, None, vp(ch), vp(cp), 2558, 8, C.byref(full)), b'above 2^32'),
               ((h, None, vp(ch), vp(cp), 92057, 6, C.byref(full)), b'above 2^32'),
               ((h, None, None, None, N - 1, D, C.byref(full)), b'must be num_envs'),
               ((h, None, None, None, 2 * N, D, C.byref(full)), b'must be num_envs'),
               ((h, None, vp(ch), None, N, D, C.byref(full)), b'hdr_in given without slot_pos_in'),
               ((h, None, None, vp(cp), N, D, C.byref(full)), b'slot_pos_in given without hdr_in'),
               ((h, eo, None, None, N, D, C.byref(full)), b'env_of'),
               ((h, None, vp(ch, 8), vp(cp), N - 1, D, C.byref(full)), b'hdr_in is not 16-byte aligned'),
               ((h, None, vp(ch), vp(cp, 2), N - 1, D, C.byref(full)), b'slot_pos_in is not 16-byte aligned'),
               ((h, None, vp(ch), vp(cp), N - 1, D, C.byref(one(hdr=vp(bufs['hdr'], 4)))), b'out->hdr is not 16-byte aligned'),
               ((h, None, vp(ch), vp(cp), N - 1, D, C.byref(one(q=vp(bufs['q']), slot_pos=vp(bufs['slot_pos'], 8)))), b'out->slot_pos is not 16-byte aligned')]
    for args, word in invalid:
        assert lib.cw_plan(*args, st) == L.CW_ERR_INVALID, word
        assert word in lib.cw_last_error(), (word, lib.cw_last_error())
    torch.cuda.synchronize()
    assert env.expand_skipped == 0
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 7. capture
def test_captured_into_a_graph_with_a_step():
    """torch.cuda.graph around step(actions) + plan(out=...) with best_action and best_q: the calls only enqueue; each replay steps the env and plans from
    the state it reaches, equal to the eager calls on a twin engine"""
    N, D = 300, 3
    names = FIELDS + ('best_action', 'best_q')
    env, keys, pos = make_env(N, *np_states(N, 93000), obs_mode='state', auto_reset=False, **K5)
    twin, _, _ = make_env(N, keys, pos, obs_mode='state', auto_reset=False, **K5)
    for e in (env, twin):
        e.reset()
        spread(e, 5, 6)
        _walk_goals(e, 3, 94)
    assert torch.equal(env.hdr, twin.hdr) and torch.equal(env.slot_pos, twin.slot_pos)
    acts = _dev(np.random.RandomState(95).randint(0, 6, N))
    out = dict(_sentinel_out(D, N), best_action=torch.full((N,), SENT, dtype=torch.uint8, device='cuda'),
               best_q=torch.full((N, 4), SENT, dtype=torch.uint8, device='cuda').view(torch.int32).squeeze(-1))
    env.plan(D, fields=names)                                                     # (warm-up outside the capture: the method's lazily built constants)
    env.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.step_async(acts)
        env.plan(D, fields=names, out=out)
    assert all(bool((t.view(torch.uint8) == SENT).all()) for t in out.values())          # (capturing ran nothing)
    for rnd in range(2):
        acts.copy_(_dev(np.random.RandomState(96 + rnd).randint(0, 6, N)))
        g.replay()
        twin.step(acts)
        eager = twin.plan(D, fields=names)
        for f in names:
            assert torch.equal(out[f], eager[f]), (rnd, f)
        assert torch.equal(env.hdr, twin.hdr)
    torch.cuda.synchronize()
    env.close()
    twin.close()
