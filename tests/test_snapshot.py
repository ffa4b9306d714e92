"""GPU tier of the device-resident snapshots: cw_snapshot_save_kernel / cw_snapshot_load_kernel through CraftingWorldVecEnv.snapshot_*.  Every load is
checked env by env with snapshot_check.check_load (itself tested on the CPU, tests/test_snapshot_logic.py) -- restored envs against their saved source,
all others byte for byte -- and the forked batch is then continued against the CPU oracle, which is brought to the same fork on the host from its OWN
values (cwo_copy from a clone of the source taken at save time, with or without the stream) and reads nothing of the engine but the actions.
Everything is bit-exact.  No timing."""
import numpy as np
import pytest
import torch

from engines import ENGINES, K5, MENUS, N1, SIZES, k_of, n_cu
from masked_check import masked_launch, spread, take
from oracle_replay import FRAMES, make_env, np_states, oracle_kw, record_steps, same, same_states, snapshot
from snapshot_check import check_load, check_save
from state_tables import oracle_frame, painted_batch
from test_masked_shapes import _engine, _width

pytestmark = pytest.mark.gpu

def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32), device='cuda')


def _step_recorded(env, acts):
    """env.step through the device tensor acts [T, N] (+ reset_envs(done) on an engine without auto-reset) -> rewards, dones [T, N]"""
    if env.auto_reset:
        return record_steps(env, acts)
    rs = torch.empty(acts.shape, dtype=torch.int32, device=acts.device)
    ds = torch.empty(acts.shape, dtype=torch.bool, device=acts.device)
    for t in range(acts.shape[0]):
        _, r, d, _ = env.step(acts[t])
        rs[t], ds[t] = r, d
        env.reset_envs(env.done)
    torch.cuda.synchronize()
    return rs.cpu().numpy(), ds.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------------------ 1. round trip and fork
CAP1 = 96
SNAPSHOT_ENGINES = dict(ENGINES, pixels_ray_auto=dict(obs_mode='pixels', raster='ray'))      # the full-frame sweep of the ray raster (tests/test_expand.py runs ENGINES)


def _rows_of_test_1():
    """-> (save_rows, load_rows): env i into row (7i + 3) mod 96 for two envs in three; envs 0-9 all from env 3's row, a permutation of the saved rows over
    envs 10-49, and among the rest -1, -7, 96, 101 and one never-saved row"""
    save = np.array([(7 * i + 3) % CAP1 if i % 3 != 2 else -1 for i in range(N1)], np.int32)
    used = save[save >= 0]
    assert len(set(used.tolist())) == len(used) == 47
    load = np.full(N1, -1, np.int32)
    load[0:10] = save[3]
    load[10:50] = np.random.RandomState(12).permutation(used)[:40]
    never = (7 * 2 + 3) % CAP1                                    # env 2's row: env 2 was not saved
    assert never not in used
    load[50:55] = [-1, -7, CAP1, 101, never]
    return save, load


def _round_trip_and_fork(engine, with_stream, S):
    from oracle import OracleBatch
    ekw, KW = dict(SNAPSHOT_ENGINES[engine]), k_of(S)
    raster, pixels, K = ekw.get('raster', 'ray'), ekw['obs_mode'] != 'state', ekw.get('fixed_init_state', 0)
    env, keys, pos = make_env(N1, *np_states(N1, 31000), **ekw, **KW)
    assert env.tuner_state()['lookahead'] == (1 if env.auto_reset else 0)
    okw = oracle_kw(dict(KW, fixed_init_state=K), raster)
    per_env = [MENUS[int(m)] for m in ekw['env_menu']] if 'env_menu' in ekw else [dict()] * N1
    ora = OracleBatch(N1, rng_states=list(zip(keys, pos)), per_env_kwargs=per_env, **okw)
    env.snapshot_reserve(CAP1)
    assert env.snapshot_row_bytes == 2577 + (196 if env.auto_reset else 0) + 18 * K
    env.reset()
    ora.reset()
    a1 = spread(env, 9, 1)
    ora.rollout(a1.astype(np.int8), nthreads=16)
    save_rows, load_rows = _rows_of_test_1()
    saved = take(env)
    pool_saved = env.fixed_states() if K else None
    o_saved = [e.clone() for e in ora.envs]                       # the oracle's own envs at save time
    env.snapshot_save(save_rows)                                  # (validated and packed on the host: vec_env.snapshot_rows)
    check_save(saved, take(env))
    a2 = spread(env, 11, 2)                                       # states move, episodes end
    ora.rollout(a2.astype(np.int8), nthreads=16)
    before = take(env)
    assert (before['state_ep_no'] > saved['state_ep_no']).any() and not np.array_equal(before['hdr'], saved['hdr'])
    rows_dev = _dev(load_rows)                                    # (96 and 101 among them: handed over in place)
    obs = env.snapshot_load(rows_dev, with_stream=with_stream)
    assert set(obs) == set(env._observation())
    after = take(env)
    good, n_bad = check_load(saved, before, after, save_rows, load_rows, with_stream, CAP1)
    assert len(good) == 50 and n_bad == 3 and env.snapshot_skipped == int(before['counters'][6]) + 3
    src = np.array([int(np.flatnonzero(save_rows == load_rows[j])[0]) for j in good])
    if K:                                                         # the pool row travels with the stream
        pool = env.fixed_states()
        want = pool_saved.copy()
        if with_stream:
            want[good] = pool_saved[src]
        same('pool', 0, pool, want)
    if 'env_menu' in ekw:
        crossing = [j for j, s in zip(good, src) if ekw['env_menu'][j] != ekw['env_menu'][s]]
        assert len(crossing) >= 5                                 # (envs 0, 2, 4, ... continue from env 3, of the other menu)
        assert np.array_equal(after['hdr'][good, 3], ekw['env_menu'][src] if with_stream else ekw['env_menu'][good])
    # ---- the oracle, brought to the same fork on the host: every restored env from the clone taken of its source at save time (cwo_copy: the episode,
    # and with the stream the stream, pool and menu too), so that whole states are compared at once, with and without the stream
    for j, s in zip(good.tolist(), src.tolist()):
        ora.envs[j].copy_from(o_saved[s], with_stream)
    same_states(env, ora, frames=tuple(FRAMES) if pixels else (), tag='right after the load: ')
    T = 2 * KW['max_steps'] + 3
    acts = torch.randint(0, 6, (T, N1), device='cuda', dtype=torch.uint8, generator=torch.Generator(device='cuda').manual_seed(3))
    r_host, d_host = _step_recorded(env, acts)
    _, o_rew, o_done = ora.rollout(acts.cpu().numpy().astype(np.int8), nthreads=16, record=True)
    same('reward of every step after the fork', 0, r_host.T, o_rew.T)
    same('done of every step after the fork', 0, d_host.T, o_done.astype(bool).T)
    assert d_host.sum(axis=0).min() >= 2                          # every env has been reset twice since, on whichever stream it continues
    same_states(env, ora, frames=tuple(FRAMES) if pixels else (), tag='%d steps after the fork: ' % T)
    env.close()


@pytest.mark.parametrize('with_stream', [True, False])
@pytest.mark.parametrize('engine', list(ENGINES))
def test_round_trip_and_fork_then_continued_against_the_oracle(engine, with_stream):
    _round_trip_and_fork(engine, with_stream, 5)


@pytest.mark.parametrize('with_stream', [True, False])
@pytest.mark.parametrize('engine,size', [(e, s) for s in SIZES for e in SNAPSHOT_ENGINES if s != 5 or e not in ENGINES])
def test_round_trip_and_fork_then_continued_against_the_oracle_at_size(engine, with_stream, size):
    """the same on 4 x 4, 7 x 7, 8 x 8 and 21 x 21 grids, and at every size on the full-frame engine of the ray raster"""
    _round_trip_and_fork(engine, with_stream, size)


# ------------------------------------------------------------------------------------------------------------------------------ 2. every dealing width
PATTERNS = ['full_chunk_beside_an_empty_one', 'last_env', 'last_partial_chunk', 'nine_in_a_row', 'nothing']


def _selected(name, N, epb, chunks):
    m = np.zeros(N, bool)
    if name == 'full_chunk_beside_an_empty_one':                  # (in the second-round case a chunk of the second round)
        c = chunks - 3
        m[c * epb:(c + 1) * epb] = True
        assert m.sum() == epb and not m[(c + 1) * epb:].any()
    elif name == 'last_env':
        m[N - 1] = True
    elif name == 'last_partial_chunk':
        m[N // epb * epb:] = True
        assert 0 < m.sum() < epb
    elif name == 'nine_in_a_row':                                 # across a chunk edge: ranks dealt over four waves in two chunks
        m[5 * epb - 4:5 * epb + 5] = True
        assert m.sum() == 9 and m[5 * epb - 1] and m[5 * epb]
    return m


@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('width', ['epb4', 'epb64', 'round2'])
def test_save_and_load_at_every_dealing_width(monkeypatch, width, pattern):
    """state mode, a bank of N rows: the selected envs are saved (env i into row N - 1 - i), move on, and are loaded back -- first the episode only, each
    from the row of the NEXT selected env, then with the stream from their own"""
    N, epb, chunks = _width(width)
    env, _, _ = _engine(monkeypatch, N, obs_mode='state', auto_reset=False, **K5)
    assert masked_launch(N, n_cu(), 1)[:2] == (epb, chunks)
    env.snapshot_reserve(N)
    env.reset()
    spread(env, 4, 6)
    sel = np.flatnonzero(_selected(pattern, N, epb, chunks))
    empty = pattern == 'nothing'
    save_rows = np.full(N, -1, np.int32)
    save_rows[sel] = N - 1 - sel
    saved = take(env)
    env.snapshot_save(_dev(save_rows))
    check_save(saved, take(env))
    spread(env, 3, 7)
    before = take(env)
    for with_stream, shift in ((False, 1), (True, 0)):
        load_rows = np.full(N, -1, np.int32)
        load_rows[sel] = save_rows[np.roll(sel, -shift)]
        env.snapshot_load(_dev(load_rows), with_stream=with_stream)
        after = take(env)
        good, n_bad = check_load(saved, before, after, save_rows, load_rows, with_stream, N, allow_empty=empty)
        assert good.tolist() == sel.tolist() and n_bad == 0
        before = after
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 3. capture
def test_save_steps_and_load_captured_in_one_graph():
    """torch.cuda.graph around snapshot_save(rows_a), step_many(5 steps), snapshot_load(rows_b) on an engine without auto-reset: capturing runs nothing,
    and three replays equal the eager sequence run three times on a twin"""
    N = 70
    rng = np.random.RandomState(5)
    rows_a = _dev(np.where(np.arange(N) % 4 == 3, -1, rng.permutation(96)[:N]))
    rows_b = rows_a[torch.as_tensor(rng.permutation(N), device='cuda')].contiguous()      # env j continues from what env perm[j] saved, or takes no part
    acts = torch.randint(0, 6, (5, N), device='cuda', dtype=torch.uint8, generator=torch.Generator(device='cuda').manual_seed(4))
    envs = []
    for _ in range(2):
        env, _, _ = make_env(N, *np_states(N, 52000), obs_mode='state', auto_reset=False, **K5)
        env.snapshot_reserve(96)
        env.reset()
        spread(env, 6, 8)
        envs.append(env)
    eager, cap = envs
    start, twin = take(cap), take(eager)
    for k in start:
        assert np.array_equal(start[k], twin[k]), k
    for _ in range(3):
        eager.snapshot_save(rows_a)
        eager.step_many(acts)
        eager.snapshot_load(rows_b)
    cap.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap.snapshot_save(rows_a)
        cap.step_many(acts)
        cap.snapshot_load(rows_b)
    torch.cuda.synchronize()
    now = take(cap)
    for k in start:
        assert np.array_equal(now[k], start[k]), 'capturing ran something: ' + k
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    want, got = take(eager), take(cap)
    assert not np.array_equal(want['hdr'], start['hdr'])
    for k in want:
        assert np.array_equal(got[k], want[k]), 'three replays against the eager sequence: ' + k
    for env in envs:
        env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 4. bank lifetime and call order
def test_bank_lifetime_and_call_order():
    from gym_craftingworld_amd import _lib as L
    N = 8
    rows = _dev(np.arange(N))
    fresh, _, _ = make_env(N, seed=3, obs_mode='state', auto_reset=False, **K5)
    fresh.snapshot_reserve(N)
    for call in (lambda: fresh.snapshot_save(rows), lambda: fresh.snapshot_load(rows)):      # a bank, but no reset yet
        with pytest.raises(L.CraftingWorldError, match=r'\(-3\)'):
            call()
    fresh.close()
    env, _, _ = make_env(N, seed=3, obs_mode='state', auto_reset=False, **K5)
    env.reset()
    assert env.snapshot_row_bytes == 0
    for call in (lambda: env.snapshot_save(rows), lambda: env.snapshot_load(rows), lambda: env.snapshot_save(np.arange(N)),
                 lambda: env.snapshot_load(envs=[1], rows=[0])):                             # reset, but no bank
        with pytest.raises(L.CraftingWorldError, match=r'\(-3\)'):
            call()
    with pytest.raises(ValueError):
        env.snapshot_reserve(-1)
    assert env.snapshot_row_bytes == 0
    env.snapshot_reserve(N)
    assert env.snapshot_row_bytes == 2577
    with pytest.raises(ValueError):
        env.snapshot_save(envs=[0, 1], rows=[N, 0])                                          # a row outside the bank: refused on the host
    spread(env, 5, 1)
    env.snapshot_save(rows)
    env.snapshot_reserve(N)                                                                  # a second reserve drops every saved row
    spread(env, 3, 2)
    before = take(env)
    env.snapshot_load(rows)
    after = take(env)
    assert after['counters'][6] == before['counters'][6] + N and env.snapshot_skipped == int(after['counters'][6])
    for k in before:
        if k != 'counters':
            assert np.array_equal(after[k], before[k]), 'a never-saved row was loaded: ' + k
    assert np.array_equal(np.delete(after['counters'], 6), np.delete(before['counters'], 6))
    env.snapshot_reserve(0)
    assert env.snapshot_row_bytes == 0
    with pytest.raises(L.CraftingWorldError, match=r'\(-3\)'):
        env.snapshot_load(rows)
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 5. the look-ahead ring
def test_the_look_ahead_ring_travels_with_the_stream():
    """auto-reset, max_steps 4: every env finishes on every fourth step and pops a record.  Saved right after such a step, run on for 3 x max_steps, loaded
    with the stream: the streams' logical positions are the saved ones and the next 3 x max_steps steps repeat what followed the save, bit for bit"""
    N, kw = 64, dict(size=(5, 5), max_steps=4)
    env, _, _ = make_env(N, *np_states(N, 64000), obs_mode='state', **kw)
    assert env.tuner_state()['lookahead'] == 1
    env.snapshot_reserve(N)
    env.reset()
    gen = torch.Generator(device='cuda').manual_seed(9)
    pre = torch.randint(0, 6, (4, N), device='cuda', dtype=torch.uint8, generator=gen)
    _, d = record_steps(env, pre)
    assert d[3].sum() > N // 2                                     # the step before the save: these envs took the record at the head of their ring
    k0, p0 = env.get_rng_states()
    s0 = take(env)
    env.snapshot_save(_dev(np.arange(N)))
    acts = torch.randint(0, 6, (3 * kw['max_steps'], N), device='cuda', dtype=torch.uint8, generator=gen)

    def run():
        out = []
        for t in range(acts.shape[0]):
            _, r, dn, _ = env.step(acts[t])
            out.append((r.clone(), dn.clone(), env.hdr.clone(), env.slot_pos.clone()))
        torch.cuda.synchronize()
        return [[x.cpu().numpy() for x in row] for row in out]
    first = run()
    before = take(env)
    env.snapshot_load(_dev(np.arange(N)))
    check_load(s0, before, take(env), np.arange(N), np.arange(N), True, N)
    k1, p1 = env.get_rng_states()
    assert np.array_equal(k1, k0) and np.array_equal(p1, p0)
    second = run()
    for t, (a, b) in enumerate(zip(first, second)):
        for name, x, y in zip(('reward', 'done', 'hdr', 'slot_pos'), a, b):
            same('%s of step %d after the load' % (name, t), 0, y, x)
    assert sum(int(row[1].sum()) for row in first) > 2 * N        # (rings drained and refilled on the way)
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 6. the resident path
def test_single_env_with_host_outputs_on_the_resident_path():
    """N = 1, host_outputs, dirty-cell frames: the resident stepper is parked by save and load, and starts again from the restored records"""
    from gym_craftingworld_amd import _lib as L
    env, _, _ = make_env(1, *np_states(1, 7100), obs_mode='pixels_dirty', auto_reset=False, host_outputs=True, size=(5, 5), max_steps=30)
    assert env.tuner_state()['resident'] == 1
    env.snapshot_reserve(2)
    env.reset()

    def step(a):
        L.check(env._lib.cw_step_resident(env._h, int(a), 0), 'cw_step_resident', env._lib)
        st = env.get_state()                                      # (parks the stepper)
        return int(env.reward[0]), bool(env.done[0]), st, env._obs.numpy().copy()
    for a in (1, 2, 4):
        step(a)
    st0, frame0, hdr0 = env.get_state(), env._obs.numpy().copy(), env.hdr.cpu().numpy().copy()
    env.snapshot_save(envs=[0], rows=[1])
    first = step(0)
    step(3)
    step(5)
    assert not np.array_equal(env.hdr.cpu().numpy(), hdr0)
    obs = env.snapshot_load(_dev([1]))
    assert np.array_equal(obs['observation'].numpy(), frame0) and np.array_equal(env.hdr.cpu().numpy(), hdr0)
    st1 = env.get_state()
    for k in st0:
        assert np.array_equal(st1[k], st0[k]), k
    again = step(0)
    assert again[:2] == first[:2] and np.array_equal(again[3], first[3])
    for k in first[2]:
        assert np.array_equal(again[2][k], first[2][k]), k
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 7. a load paints every state class
N7 = 48
PAINT_CASES = [('pixels_dirty', 5), ('pixels_dirty', 8), ('pixels_dirty', 21), ('pixels', 8), ('pixels', 21)]


def _oracle_frames(grid, agent, hold, alt):
    return np.stack([oracle_frame(grid[j], agent[j], hold[j], alt) for j in range(len(grid))])


@pytest.mark.parametrize('obs_mode,size', PAINT_CASES)
@pytest.mark.parametrize('raster', ['ray', 'alt'])
def test_a_load_paints_every_state_class(raster, obs_mode, size):
    """cw_snapshot_load_kernel<true> repaints the three frames of an env.  The states are state_tables.painted_states -- every hold on an empty cell and over
    an object, sticks over sticks (the alt raster's doubled pixel), bread made, a house, rock and bread gone, every corner, cells 0 and S*S - 1 -- injected,
    saved, stepped away from and loaded into the neighbouring env: the painted frames against the oracle's rasteriser on the injected states, not against
    frames the engine painted earlier.  The full-frame engines sweep once more after a Drop."""
    from expand_check import oracle_successors
    N, S, alt = N7, size, raster == 'alt'
    names, grid, init, agent, hold = painted_batch(S, N)
    env, _, _ = make_env(N, *np_states(N, 58000), obs_mode=obs_mode, raster=raster, auto_reset=False, **k_of(S))
    env.snapshot_reserve(N)
    env.reset()
    env.set_state(grid=grid, init_grid=init, agent_rc=agent, init_agent_rc=agent, hold=hold, step_num=np.full(N, 3, np.int32))
    want_obs, want_init = _oracle_frames(grid, agent, hold, alt), _oracle_frames(init, agent, np.zeros(N, np.uint8), alt)
    saved = take(env)
    same('observation of the injected states', 0, saved['observation'], want_obs)
    same('init_observation of the injected states', 0, saved['init_observation'], want_init)
    save_rows = (N - 1 - np.arange(N)).astype(np.int32)
    env.snapshot_save(_dev(save_rows))
    check_save(saved, take(env))
    spread(env, 6, 3)
    before = take(env)
    assert (before['observation'] != saved['observation']).reshape(N, -1).any(axis=1).sum() > N // 2
    nxt = (np.arange(N) + 1) % N                                   # env i continues from what env i + 1 saved
    load_rows = save_rows[nxt]
    obs = env.snapshot_load(_dev(load_rows), with_stream=True)
    after = take(env)
    good, n_bad = check_load(saved, before, after, save_rows, load_rows, True, N)
    assert len(good) == N and n_bad == 0
    for j in np.flatnonzero((after['observation'] != want_obs[nxt]).reshape(N, -1).any(axis=1))[:4]:
        print('observation of env %d differs: %s' % (j, names[nxt[j]]))
    same('observation painted by the load', 0, obs['observation'].cpu().numpy(), want_obs[nxt])
    same('init_observation painted by the load', 0, obs['init_observation'].cpu().numpy(), want_init[nxt])
    same('desired_goal painted by the load', 0, after['desired_goal'], saved['desired_goal'][nxt])
    if obs_mode == 'pixels':                                       # one sweep from the restored records
        z = np.zeros(N, np.int64)
        dense = dict(grid=grid[nxt], agent=agent[nxt].astype(np.int64), hold=hold[nxt].astype(np.int64), achieved=z, desired=z + 1, step_num=z + 3, flags=z)
        suc = oracle_successors(dense, init[nxt], k_of(S))
        assert 4 <= suc['changed'][5].sum() < N                    # (the oracle alone: some drop what they hold, most cannot)
        env.step(torch.full((N,), 5, dtype=torch.uint8, device='cuda'))
        same('the frame swept after a Drop', 0, env._observation()['observation'].cpu().numpy(),
             _oracle_frames(suc['grid'][5], suc['agent'][5], suc['hold'][5], alt))
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 8. large grids
@pytest.mark.parametrize('raster', ['ray', 'alt'])
@pytest.mark.parametrize('S', [182, 255])
def test_save_and_load_on_large_grids(S, raster):
    """182 x 182 and 255 x 255, dirty-cell frames: agents in the far corners (rows and columns up to 254 in the header bytes), slot cells above 32 767, held and
    gone marks.  Saved, stepped, loaded without the stream from the neighbour's row and with it from the env's own; the painted frames against the
    oracle's rasteriser; three more steps against an OracleBatch brought to the same states by reset + set_state."""
    from oracle import OracleBatch
    N, alt = 6, raster == 'alt'
    KW = dict(size=(S, S), max_steps=50)
    names, grid, _, agent, hold = painted_batch(S, 22)
    far = [j for j in range(22) if names[j].startswith('corner') and max(agent[j]) >= 128]
    assert len(far) == N and sorted(hold[far].tolist()) == [0, 0, 0, 1, 2, 3]
    grid, agent, hold = grid[far], agent[far], hold[far]
    env, keys, pos = make_env(N, *np_states(N, 59000), obs_mode='pixels_dirty', raster=raster, auto_reset=False, **KW)
    ora = OracleBatch(N, rng_states=list(zip(keys, pos)), **oracle_kw(KW, raster))
    env.snapshot_reserve(N)
    env.reset()
    ora.reset()
    same_states(env, ora, frames=tuple(FRAMES), tag='after the reset: ')
    start = env.get_state()
    env.set_state(grid=grid, agent_rc=agent, hold=hold)
    want_obs = _oracle_frames(grid, agent, hold, alt)
    saved = take(env)
    assert (saved['slot_pos'] < -2).sum() >= N                     # cells above 32 767: negative in the int16 tensor
    same('observation of the injected states', 0, saved['observation'], want_obs)
    save_rows = (N - 1 - np.arange(N)).astype(np.int32)
    env.snapshot_save(_dev(save_rows))
    check_save(saved, take(env))
    spread(env, 4, 5)
    before = take(env)
    assert not np.array_equal(before['hdr'], saved['hdr'])
    nxt = (np.arange(N) + 1) % N
    for with_stream, src in ((False, nxt), (True, np.arange(N))):
        load_rows = save_rows[src]
        env.snapshot_load(_dev(load_rows), with_stream=with_stream)
        after = take(env)
        good, n_bad = check_load(saved, before, after, save_rows, load_rows, with_stream, N)
        assert len(good) == N and n_bad == 0
        same('observation painted by the load', 0, after['observation'], want_obs[src])
        for k, g, a in (('init_observation', 'init_grid', 'init_agent_rc'), ('desired_goal', 'goal_grid', 'goal_agent_rc')):
            same(k + ' painted by the load', 0, after[k], _oracle_frames(start[g][src], start[a][src], np.zeros(N, np.uint8), alt))
        before = after
    for j, e in enumerate(ora.envs):                               # the oracle: its own episode, the injected state
        v = e.view()
        e.set_state(grid[j], e.state()['init_grid'], agent[j], hold[j], v.achieved, v.desired, v.step_num)
    acts = torch.randint(0, 6, (3, N), device='cuda', dtype=torch.uint8, generator=torch.Generator(device='cuda').manual_seed(6))
    r_host, d_host = _step_recorded(env, acts)
    _, o_rew, o_done = ora.rollout(acts.cpu().numpy().astype(np.int8), nthreads=N, record=True)
    same('reward of the steps after the load', 0, r_host.T, o_rew.T)
    same('done of the steps after the load', 0, d_host.T, o_done.astype(bool).T)
    snap = snapshot(env, frames=tuple(FRAMES))
    same_ep = np.flatnonzero(~d_host.any(axis=0))                  # (the oracle's set_state forgets the agent's start cell until its next reset: there the
    assert len(same_ep) >= N // 2                                  #  engine's is compared with what the reset gave, which the oracle has confirmed)
    same('init_agent_rc', same_ep, snap['init_agent_rc'][same_ep], start['init_agent_rc'][same_ep])
    snap['init_agent_rc'] = snap['init_agent_rc'].astype(np.int64)
    snap['init_agent_rc'][same_ep] = -1
    same_states(snap, ora, frames=tuple(FRAMES), tag='3 steps after the load: ')
    env.close()
