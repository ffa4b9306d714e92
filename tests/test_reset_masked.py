"""GPU tier of the partial reset: cw_reset_masked (cw_reset_masked_kernel) through CraftingWorldVecEnv.reset_envs and the adaptors, bit-exact against the
CPU oracle.  A masked reset is reset() of each selected env, which the oracle already does one env at a time; and an auto_reset=False engine that calls
reset_envs(env.done) after every step must compute exactly what the oracle's auto-reset rollout computes, so the big comparisons go through
oracle_replay.replay_against_oracle as it is.  No timing is asserted here (tests/test_zz_reset_masked_perf.py)."""
import numpy as np
import pytest
import torch

from oracle_replay import (FRAMES, assert_counters, compare_with_oracle, make_env, np_states, oracle_kw, replay_against_oracle, same_states, set_phase,
                           snapshot)

pytestmark = pytest.mark.gpu

_BUFFERS = ('reward', 'done', 'achieved_mask', 'desired_mask', 'episode_length', 'episode_return', 'hdr', 'slot_pos', 'counters', 'terminal_observation')


def _buffers(env):
    """every buffer of cw_buffer_table as numpy arrays (frames included in the pixel modes)"""
    out = {k: getattr(env, k).cpu().numpy().copy() for k in _BUFFERS if getattr(env, k) is not None}
    if env.obs_mode != 'state':
        for k in FRAMES:
            out[k] = env._observation()[k].cpu().numpy().copy()
    return out


def _everything(env):
    """... plus get_state() and the RNG states"""
    out = _buffers(env)
    out.update(('state_' + k, v) for k, v in env.get_state().items())
    out['rng_key'], out['rng_pos'] = env.get_rng_states()
    return out


def _assert_same(a, b, rows=None, tag=''):
    assert set(a) == set(b)
    for k in a:
        x, y = (a[k], b[k]) if rows is None or k == 'counters' else (a[k][rows], b[k][rows])
        assert np.array_equal(x, y), tag + k


def _start_cell_forgotten(snap, rows):
    """The oracle's cwo_set_state -- set_phase, compare_with_oracle(phase=...) -- forgets an env's start cell ("injected states carry no agent start
    cell": its view shows (-1, -1)) until the env's next reset.  -> the snapshot with that marker in `rows`, the envs not reset since: the comparison
    then holds for every env what the oracle knows of it, and the caller checks the engine's own start cells of `rows` against values compared earlier
    (the INIT_OBS frames, compared for every env, show the start cell too)."""
    snap = dict(snap)
    rc = snap['init_agent_rc'].astype(np.int64)
    rc[rows] = -1
    snap['init_agent_rc'] = rc
    return snap


def _manual_reset_loop(env, acts):
    """step, then reset_envs(env.done) -- the engine's own buffer, in place -- after every step -> (rewards, dones) of every step, read once"""
    rs = torch.empty(acts.shape, dtype=torch.int32, device=acts.device)
    ds = torch.empty(acts.shape, dtype=torch.bool, device=acts.device)
    for t in range(acts.shape[0]):
        _, r, d, _ = env.step(acts[t])
        rs[t] = r
        ds[t] = d
        env.reset_envs(env.done)
    torch.cuda.synchronize()
    return rs.cpu().numpy(), ds.cpu().numpy()


# ------------------------------------------------------------------ A
@pytest.mark.parametrize('obs_mode,raster,style,finished,successes',
                         [('state', 'ray', None, 1955, 206), ('pixels', 'ray', 'subset', 1960, 228), ('pixels_dirty', 'ray', None, 1955, 206),
                          ('pixels', 'alt', None, 1955, 206), ('pixels_dirty', 'alt', 'subset', 1960, 228)])
def test_manual_reset_of_finished_envs_equals_the_oracles_auto_reset(obs_mode, raster, style, finished, successes):
    """auto_reset=False + reset_envs(env.done) after every step == the oracle's auto-reset rollout: every reward and done of 70 steps, and at the end state,
    episode counts, frames and RNG of every env.  For these inputs the oracle finishes 1 955 episodes (206 successes) under the equality rule and 1 960
    (228) under 'subset', the mask is a proper non-empty subset of the batch on 68 of the 70 steps and every env is reset 5 to 8 times."""
    N = 384
    kw = dict(size=(5, 5), max_steps=14, selected_tasks=['MoveAxe', 'MoveSticks', 'GoToHouse', 'EatBread'], number_of_tasks=1, reward_style=style)
    env, keys, pos = make_env(N, *np_states(N, 31000), obs_mode=obs_mode, raster=raster, auto_reset=False, **kw)
    env.reset()
    acts = np.random.RandomState(5).randint(0, 6, (70, N))
    r_host, d_host = _manual_reset_loop(env, torch.as_tensor(acts, device=env.device))
    res = replay_against_oracle(env, keys, pos, oracle_kw(kw, raster), acts, r_host, d_host, frames=obs_mode != 'state')
    assert (res['finished'], res['successes']) == (finished, successes)
    proper = (d_host.sum(axis=1) > 0) & (d_host.sum(axis=1) < N)
    assert int(proper.sum()) == 68 and res['done_per_env'].min() == 5 and res['done_per_env'].max() == 8
    assert_counters(env, N, 70, res)                         # (the STEPS counted the finishes; the masked resets added nothing)
    assert env.tuner_state()['lookahead'] == 0
    env.close()


# ------------------------------------------------------------------ B
def test_manual_reset_at_full_size_with_full_frames_against_the_oracle():
    """65 536 envs, 21x21, full frames, auto_reset=False, episode phases spread by 7 (coprime to max_steps = 300): 218 or 219 envs time out on EVERY step
    (plus the odd success), so every one of the 64 masks is sparse and non-empty.  State, episode count, RNG and the three frame arrays of every env."""
    N, T = 65536, 64
    kw = dict(size=(21, 21), max_steps=300)
    env, keys, pos = make_env(N, obs_mode='pixels', seed=314, auto_reset=False, **kw)
    phase = ((np.arange(N) * 7) % 300).astype(np.int32)
    env.reset()
    env.set_state(step_num=phase)
    start = env.get_state()
    assert np.array_equal(start['init_agent_rc'], start['agent_rc'])
    acts = torch.randint(0, 6, (T, N), device='cuda', dtype=torch.uint8, generator=torch.Generator(device='cuda').manual_seed(12))
    r_host, d_host = _manual_reset_loop(env, acts)
    per_step = d_host.sum(axis=1)
    assert per_step.min() > 0 and per_step.max() < 1000      # (every mask non-empty and sparse: 218 or 219 time-outs by construction, give or take the successes)
    snap = snapshot(env, None, tuple(FRAMES))
    never = ~d_host.any(axis=0)                              # (most envs: 64 steps of episodes of 300)
    assert np.array_equal(snap['init_agent_rc'][never], start['init_agent_rc'][never])
    res = compare_with_oracle(_start_cell_forgotten(snap, never), keys, pos, kw, acts.cpu().numpy(), r_host, d_host, phase=phase)
    assert res['finished'] == int(env.counters[1].item()) and res['finished'] >= 64 * 218
    env.close()


# ------------------------------------------------------------------ C
_TWO_MENUS = [dict(selected_tasks=['MoveAxe', 'EatBread', 'ChopTree'], number_of_tasks=2), dict(selected_tasks=['GoToHouse', 'MoveSticks'], stacking=False,
                                                                                                reward_style='subset')]


@pytest.mark.parametrize('obs_mode,raster,extra', [('state', 'ray', 'pool'), ('pixels', 'ray', 'menus'), ('pixels_dirty', 'ray', None),
                                                   ('pixels_dirty', 'alt', 'pool')])
def test_forced_resets_on_a_look_ahead_engine_in_lock_step_with_the_oracle(obs_mode, raster, extra):
    """auto_reset=True (finished envs take look-ahead records inside the step) and, after every step, a forced reset of a seeded Bernoulli(0.1) choice of
    envs through a device mask, on every 8th step one more through indices=; the oracle resets the same envs.  Forced resets are in none of counters[0..3]."""
    from oracle import OracleBatch
    N, T = 512, 60
    kw = dict(size=(6, 6), max_steps=20)
    if extra == 'pool':
        kw['fixed_init_state'] = 3
    env_menu = (np.arange(N) % 3 == 0).astype(np.uint8)
    ekw = dict(task_menus=_TWO_MENUS, env_menu=env_menu) if extra == 'menus' else {}
    env, keys, pos = make_env(N, *np_states(N, 8800), obs_mode=obs_mode, raster=raster, **kw, **ekw)
    ora = OracleBatch(N, rng_states=list(zip(keys, pos)), per_env_kwargs=[_TWO_MENUS[m] for m in env_menu] if extra == 'menus' else None,
                      **oracle_kw(kw, raster))
    assert env.tuner_state()['lookahead'] == 1
    env.reset()
    ora.reset()
    rng = np.random.RandomState(77)
    acts = rng.randint(0, 6, (T, N)).astype(np.int32)
    dacts = torch.as_tensor(acts, device=env.device)
    frames = tuple(FRAMES) if obs_mode != 'state' else ()
    res = dict(finished=0, successes=0)
    forced = 0
    for t in range(T):
        _, rew, done, _ = env.step(dacts[t])
        o_rew, o_done = ora.step(acts[t])
        assert np.array_equal(rew.cpu().numpy(), o_rew) and np.array_equal(done.cpu().numpy(), o_done), t
        res['finished'] += int(o_done.sum())
        res['successes'] += int((o_rew == 20).sum())
        mask = rng.rand(N) < 0.1
        env.reset_envs(torch.as_tensor(mask, device=env.device))
        for i in np.nonzero(mask)[0]:
            ora.envs[i].reset()
        forced += int(mask.sum())
        if t % 8 == 7:
            idx = rng.randint(-N, N, 9).tolist()
            idx.append(idx[0])                                  # (a duplicate: one reset)
            env.reset_envs(indices=idx)
            for i in sorted({i % N for i in idx}):
                ora.envs[i].reset()
        if t % 10 == 9 or t == T - 1:
            same_states(env, ora, frames=frames, tag='step %d: ' % t)
    assert forced > 2000 and res['finished'] > N // 4 and res['successes'] > 0
    assert_counters(env, N, T, res)
    env.close()


# ------------------------------------------------------------------ D
@pytest.mark.parametrize('obs_mode', ['state', 'pixels_dirty'])
def test_ring_accounting_of_forced_resets(obs_mode):
    """An env's ring holds CW_LA_DEPTH = 4 look-ahead records; counters[5] counts the resets that found none (craftingworld.h).  Right after reset() every ring
    is full: four masked resets of the same 40 envs find records, the fifth and sixth are reset from their streams.  A refill rides on every
    max_steps / 4 = 50th step at the latest and tops the QUEUED rings up: after 64 counted no-ops (action id 6: step_num += 1, reward -1 -- nothing can
    finish and take a record) four more masked resets find records again and the fifth does not.  State, frames and RNG equal the oracle's all the way."""
    from oracle import OracleBatch
    N = 256
    kw = dict(size=(6, 6), max_steps=200)
    env, keys, pos = make_env(N, *np_states(N, 4100), obs_mode=obs_mode, **kw)
    ora = OracleBatch(N, rng_states=list(zip(keys, pos)), **kw)
    assert env.tuner_state()['lookahead'] == 1
    env.reset()
    ora.reset()
    frames = tuple(FRAMES) if obs_mode != 'state' else ()
    sel = np.sort(np.random.RandomState(3).choice(N, 40, replace=False))
    mask = torch.zeros(N, dtype=torch.bool, device=env.device)
    mask[torch.as_tensor(sel, device=env.device)] = True
    slow = lambda: int(env._counters_raw[5].item())          # noqa: E731

    def forced(expect):
        env.reset_envs(mask)
        for i in sel:
            ora.envs[i].reset()
        assert slow() == expect, (slow(), expect)

    base = slow()
    for k in range(6):
        forced(base + 40 * max(0, k - 3))
    six = snapshot(env, None, frames)
    same_states(six, ora, frames=frames, tag='after six forced resets: ')
    noop = torch.full((N,), 6, dtype=torch.int32, device=env.device)
    for _ in range(64):
        _, rew, done, _ = env.step(noop)
    assert bool((rew == -1).all()) and not bool(done.any()) and slow() == base + 80
    set_phase(ora, [e.view().step_num + 64 for e in ora.envs])          # (the oracle's step refuses action 6: its 64 no-ops are step_num += 64)
    snap = snapshot(env, None, frames)
    assert np.array_equal(snap['init_agent_rc'], six['init_agent_rc'])
    same_states(_start_cell_forgotten(snap, np.arange(N)), ora, frames=frames, tag='after 64 no-ops: ')
    for k in range(5):
        forced(base + 80 + 40 * max(0, k - 3))
    snap = snapshot(env, None, frames)
    rest = np.setdiff1d(np.arange(N), sel)
    assert np.array_equal(snap['init_agent_rc'][rest], six['init_agent_rc'][rest])
    same_states(_start_cell_forgotten(snap, rest), ora, frames=frames, tag='after five more: ')
    c = env.counters.cpu().numpy()
    assert (int(c[0]), int(c[1]), int(c[2]), int(c[3])) == (64 * N, 0, 0, 64 * N)
    env.close()


# ------------------------------------------------------------------ E
@pytest.mark.parametrize('obs_mode,auto_reset', [('state', True), ('pixels', True), ('pixels_dirty', True), ('pixels_dirty', False)])
def test_unselected_rows_are_untouched(obs_mode, auto_reset):
    """An all-zero mask changes nothing at all; a mask selecting one env changes that row only -- every buffer of cw_buffer_table, counters[0..3], get_state()
    and the RNG states are byte-identical before and after in every other row; the selected row's reward, done and episode statistics stay too."""
    N = 200
    kw = dict(size=(7, 7), max_steps=9, obs_mode=obs_mode, auto_reset=auto_reset, keep_terminal_obs=auto_reset and obs_mode != 'state')
    env, _, _ = make_env(N, *np_states(N, 66), **kw)
    env.reset()
    acts = torch.as_tensor(np.random.RandomState(2).randint(0, 6, (30, N)), device=env.device)
    for t in range(30):
        env.step(acts[t])
    before = _everything(env)
    j = int(np.nonzero(before['state_step_num'] > 0)[0][100])       # (an env in the middle of an episode)
    assert before['counters'][1] > N and (before['terminal_observation'].any() if 'terminal_observation' in before else True)
    raw = env._counters_raw.cpu().numpy().copy()
    env.reset_envs(torch.zeros(N, dtype=torch.uint8, device=env.device))
    _assert_same(_everything(env), before, tag='all-zero mask: ')
    assert np.array_equal(env._counters_raw.cpu().numpy(), raw)
    env.reset_envs(indices=[])
    _assert_same(_everything(env), before, tag='no indices: ')
    one = torch.zeros(N, dtype=torch.bool, device=env.device)
    one[j] = True
    env.reset_envs(one)
    after = _everything(env)
    others = np.arange(N) != j
    _assert_same(after, before, rows=others, tag='one env: ')
    for k in ('reward', 'done', 'episode_length', 'episode_return') + (('terminal_observation',) if 'terminal_observation' in before else ()):
        assert np.array_equal(after[k][j], before[k][j]), k
    assert after['state_step_num'][j] == 0 and before['state_step_num'][j] > 0 and after['state_ep_no'][j] == before['state_ep_no'][j] + 1
    assert after['achieved_mask'][j] == 0 and after['desired_mask'][j] == after['state_desired'][j].astype(np.int16)
    assert np.array_equal(after['state_grid'][j], after['state_init_grid'][j])
    if obs_mode != 'state':
        assert np.array_equal(after['observation'][j], after['init_observation'][j])
    env.close()


# ------------------------------------------------------------------ F
@pytest.mark.parametrize('obs_mode,raster,auto_reset', [('state', 'ray', True), ('pixels', 'ray', True), ('pixels_dirty', 'ray', False), ('pixels', 'alt', False),
                                                        ('pixels_dirty', 'alt', True)])
def test_all_ones_mask_equals_reset(obs_mode, raster, auto_reset):
    """Two engines, same seed, same 30 steps; one reset(), the other reset_envs(ones): all buffers, states and RNG equal, and equal again 20 steps later."""
    from gym_craftingworld_amd import CraftingWorldVecEnv
    N = 700
    kw = dict(size=(8, 8), max_steps=11, obs_mode=obs_mode, raster=raster, auto_reset=auto_reset, seed=91)
    a, b = CraftingWorldVecEnv(N, **kw), CraftingWorldVecEnv(N, **kw)
    acts = torch.as_tensor(np.random.RandomState(6).randint(0, 6, (50, N)), device=a.device)
    for e in (a, b):
        e.reset()
        for t in range(30):
            e.step(acts[t])
    a.reset()
    b.reset_envs(torch.ones(N, dtype=torch.uint8, device=b.device))
    _assert_same(_everything(b), _everything(a), tag='after the reset: ')
    for e in (a, b):
        for t in range(30, 50):
            e.step(acts[t])
    _assert_same(_everything(b), _everything(a), tag='20 steps later: ')
    a.close()
    b.close()


# ------------------------------------------------------------------ G
def test_masked_reset_and_steps_captured_into_one_graph():
    """torch.cuda.graph around reset_envs(mask) + step_many(actions) on an auto_reset=False state-mode engine: the call only enqueues, so it is captured
    with the steps; five replays with the mask (the last replay's done) and the actions rewritten in place equal an eager twin.  One stream."""
    from gym_craftingworld_amd import CraftingWorldVecEnv
    N, K = 2048, 6
    kw = dict(size=(6, 6), max_steps=8, obs_mode='state', auto_reset=False, seed=17)
    eager, graphed = CraftingWorldVecEnv(N, **kw), CraftingWorldVecEnv(N, **kw)
    eager.reset()
    graphed.reset()
    mask_t = torch.zeros(N, dtype=torch.bool, device='cuda')
    ring = torch.zeros((K, N), dtype=torch.uint8, device='cuda')
    graphed.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graphed.reset_envs(mask_t)
        graphed.step_many(ring)
    assert int(graphed.counters[0]) == 0                     # (capturing ran nothing)
    gen = torch.Generator(device='cuda').manual_seed(33)
    selected = 0
    for r_ in range(5):
        acts = torch.randint(0, 6, (K, N), device='cuda', dtype=torch.uint8, generator=gen)
        if r_:
            mask_t.copy_(graphed.done)
        selected += int(mask_t.sum())
        ring.copy_(acts)
        g.replay()
        eager.reset_envs(mask_t.clone())
        for t in range(K):
            eager.step(acts[t])
        assert torch.equal(graphed.reward, eager.reward) and torch.equal(graphed.done, eager.done), r_
    assert selected > N
    assert torch.equal(graphed.hdr, eager.hdr) and torch.equal(graphed.slot_pos, eager.slot_pos) and torch.equal(graphed.counters, eager.counters)
    torch.cuda.synchronize()
    _assert_same(_everything(graphed), _everything(eager))
    eager.close()
    graphed.close()


# ------------------------------------------------------------------ H
@pytest.mark.parametrize('obs_mode,auto_reset', [('pixels_dirty', True), ('state', False)])
def test_checkpoint_between_masked_resets(obs_mode, auto_reset, tmp_path):
    """masked resets, save_checkpoint, 20 steps with masked resets, load_checkpoint, the same 20 steps: identical buffers, state and RNG."""
    N = 300
    env, _, _ = make_env(N, *np_states(N, 1234), size=(6, 6), max_steps=10, obs_mode=obs_mode, auto_reset=auto_reset)
    env.reset()
    rng = np.random.RandomState(4)
    acts = torch.as_tensor(rng.randint(0, 6, (35, N)), device=env.device)
    masks = [torch.as_tensor(rng.rand(N) < 0.15, device=env.device) for _ in range(35)]

    def run(lo, hi):
        for t in range(lo, hi):
            env.step(acts[t])
            env.reset_envs(masks[t] | env.done if not auto_reset else masks[t])

    run(0, 15)
    path = str(tmp_path / 'masked.ckpt')
    env.save_checkpoint(path)
    run(15, 35)
    first = _everything(env)
    env.load_checkpoint(path)
    run(15, 35)
    _assert_same(_everything(env), first)
    assert first['counters'][1] > 0
    env.close()


# ------------------------------------------------------------------ I
def test_errors_and_adaptors():
    from gym_craftingworld_amd import CraftingWorldVecEnv
    from gym_craftingworld_amd._lib import CraftingWorldError
    from gym_craftingworld_amd.adapters import GymnasiumVecAdapter, MultiDeviceVecEnv
    N = 300
    kw = dict(size=(5, 5), max_steps=15, obs_mode='pixels_dirty')
    keys, pos = np_states(N, 909)
    acts = torch.as_tensor(np.random.RandomState(1).randint(0, 6, (20, N)).astype(np.int32), device='cuda')
    mask = np.random.RandomState(2).rand(N) < 0.3
    single = CraftingWorldVecEnv(N, **kw)
    single.set_rng_states(keys, pos)
    with pytest.raises(CraftingWorldError):                      # CW_ERR_STATE: no cw_reset yet
        single.reset_envs(torch.zeros(N, dtype=torch.bool, device='cuda'))
    single.reset()
    for bad in (torch.zeros(N - 1, dtype=torch.bool, device='cuda'), torch.zeros(N, dtype=torch.bool), torch.zeros((N, 1), dtype=torch.uint8, device='cuda')):
        with pytest.raises(ValueError):
            single.reset_envs(bad)
    with pytest.raises(ValueError):
        single.reset_envs(torch.zeros(N, dtype=torch.bool, device='cuda'), indices=[0])
    with pytest.raises(ValueError):
        single.reset_envs()
    with pytest.raises(IndexError):
        single.reset_envs(indices=[N])
    # the adaptors and a host_outputs engine against `single`
    twin = CraftingWorldVecEnv(N, **kw)
    twin.set_rng_states(keys, pos)
    ga = GymnasiumVecAdapter(twin)
    ga.reset()
    multi = MultiDeviceVecEnv(N, ['cuda:0', 'cuda:0'], **kw)
    multi.set_rng_states(keys, pos)
    multi.reset()
    host = CraftingWorldVecEnv(N, host_outputs=True, **kw)
    host.set_rng_states(keys, pos)
    host.reset()
    a_host = acts.cpu().numpy()
    for t in range(20):
        single.step(acts[t])
        ga.step(acts[t])
        multi.step(acts[t])
        host.step(a_host[t])
    with pytest.raises(ValueError):                              # (re-seeding restarts every env's stream)
        ga.reset(seed=3, options={'reset_mask': mask})
    want = single.reset_envs(mask=mask)
    obs, info = ga.reset(options={'reset_mask': torch.as_tensor(mask, device='cuda')})
    outs = multi.reset_envs(mask)
    multi.synchronize()
    h_obs = host.reset_envs(mask)                                # (synchronised on return, CPU tensors)
    assert not h_obs['observation'].is_cuda
    for k in FRAMES:
        assert torch.equal(obs[k], want[k]) and torch.equal(torch.cat([o[k] for o in outs]), want[k]) and torch.equal(h_obs[k], want[k].cpu()), k
    assert torch.equal(info['desired_goal'], single.hdr[:, 6:8])
    for t in range(10):
        single.step(acts[t])
        ga.step(acts[t])
        multi.step(acts[t])
        host.step(a_host[t])
    multi.synchronize()
    ref = _everything(single)
    _assert_same(_everything(twin), ref, tag='gymnasium adaptor: ')
    _assert_same(_everything(host), ref, tag='host_outputs: ')
    lo = 0
    for sh in multi.shards:
        got = _everything(sh)
        for k in ('hdr', 'slot_pos', 'observation', 'desired_goal', 'init_observation', 'rng_key', 'rng_pos', 'reward', 'done'):
            assert np.array_equal(got[k], ref[k][lo:lo + sh.num_envs]), ('multi-device', k)
        lo += sh.num_envs
    assert sum(int(sh.counters[1]) for sh in multi.shards) == int(single.counters[1]) > 0
    ga.close()
    multi.close()
    host.close()
    single.close()
