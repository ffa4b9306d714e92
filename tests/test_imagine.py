"""GPU tier of the goal-drawing feature: cw_imagine_masked / cw_sample_state_masked (cw_imagine_masked_kernel, cw_sample_state_masked_kernel) through
CraftingWorldVecEnv.imagine_obs / .sample_states, MultiDeviceVecEnv and the N=1 classes.  Everything is bit-exact: the comparator is the numpy model of
tests/imagine_model.py, which tests/test_imagine_model.py pins to fixtures captured from the reference; frames come from the oracle's rasterisers; what
follows a committed goal is compared with the CPU oracle, the new desired mask injected as oracle_replay.set_phase injects a phase.  No timing."""
import ctypes as C

import numpy as np
import pytest
import torch

import imagine_model as M
from masked_check import device_side as _device_side, model_imagine as _model, spread as _spread
from oracle_replay import make_env, np_states, oracle_arrays, oracle_kw, same

pytestmark = pytest.mark.gpu

TASKS = ['MakeBread', 'EatBread', 'BuildHouse', 'ChopTree', 'ChopRock', 'GoToHouse', 'MoveAxe', 'MoveHammer', 'MoveSticks']
_MENUS8 = [dict(), dict(selected_tasks=TASKS[::-1]), dict(selected_tasks=TASKS[:4], number_of_tasks=2),
           dict(selected_tasks=['GoToHouse', 'MoveAxe', 'EatBread'], stacking=False), dict(selected_tasks=TASKS[3:], reward_style='subset'),
           dict(selected_tasks=['ChopTree', 'BuildHouse'], number_of_tasks=1), dict(selected_tasks=TASKS[1::2]),
           dict(selected_tasks=TASKS[::2], number_of_tasks=3, reward_style='subset')]
CLASSES = {'CraftingWorldEnvRay': 'CraftingWorldEnv', 'CraftingWorldEnvFlat': 'CraftingWorldEnvFlat', 'CraftingWorldEnvOneHot': 'CraftingWorldEnvOneHot',
           'CraftingWorldEnvAltObs': 'CraftingWorldEnvAltObs'}


# ------------------------------------------------------------------------------------------------------------------------------ helpers
def _frames_equal(got, rows, grids, agents, alt, what):
    """device frames got[rows] == the oracle's render of the model's goal states, in chunks (a 65 536-env frame array is 1.4 GB)"""
    for lo in range(0, len(rows), 4096):
        sl = slice(lo, lo + 4096)
        want = np.stack([M.render(grids[j], agents[j], alt) for j in range(lo, min(lo + 4096, len(rows)))])
        have = got[torch.as_tensor(rows[sl], device=got.device)].cpu().numpy()
        same(what, rows[sl], have, want)


def _rows_equal(a, b, rows, tag):
    r = None if rows is None else torch.as_tensor(rows, device=a['hdr'].device)
    for k in a:
        x, y = (a[k], b[k]) if r is None or k == 'counters' else (a[k][r], b[k][r])
        assert torch.equal(x, y), tag + k


def _state_equal(st, st0, rows, skip=()):
    for k in st:
        if k not in skip:
            assert np.array_equal(st[k][rows], st0[k][rows]), k


# ------------------------------------------------------------------------------------------------------------------------------ (1) the fixtures, N = 1
@pytest.mark.parametrize('reference_dtypes', [False, True])
@pytest.mark.parametrize('resident', [True, False])
@pytest.mark.parametrize('name', M.fixture_names())
def test_fixtures_through_the_hip_engine(name, resident, reference_dtypes):
    """the op scripts captured from the reference, through the N=1 classes on the resident and the launch path, uint8 and reference dtypes: every returned
    array by CRC / dtype / shape, new objects, np_random (mirror, caller's draws, caller's RandomState) after every op, get_rng_state() after every
    imagine_obs, desired_goal and INIT_OBS_VECTOR untouched"""
    import gym_craftingworld_amd.env as E
    meta, kw, d = M.load(name)
    ck = dict(meta['ctor_kwargs'])
    if 'size' in ck:
        ck['size'] = tuple(ck['size'])
    env = getattr(E, CLASSES[meta['env']])(reference_dtypes=reference_dtypes, resident=resident, **ck)
    env.set_rng_state(d['key0'], int(d['pos0']))
    if ck.get('fixed_init_state'):
        env.generate_fixed_states()
    streams = []

    def probe(e, ret):
        k, p = e.get_rng_state()
        streams.append((int(p), M.crc(np.asarray(k, np.uint32))))
        return None
    rows, _ = M.run_script(env, d['ops'], d['args'], probe)
    want = d['rows'].copy()
    img = d['ops'] == M.I_IMAGINE
    want[img, M.COL_STATE], want[img, M.COL_AGENT] = 0, 0      # (the Ray classes return pixels: the goal state itself is compared in the batch tests)
    if not reference_dtypes:
        want[img, M.COL_DTYPE] = 1 * 4 + 1                     # uint8 unless the caller asked for the reference's int64
    for i in range(len(rows)):
        assert np.array_equal(rows[i], want[i]), 'op %d (%d, arg %d): engine %s, reference %s' % (i, d['ops'][i], d['args'][i], rows[i], want[i])
    assert streams == [(int(r[M.COL_POS]), int(r[M.COL_KEY])) for r in d['rows'][img]]
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ (2) the batch
@pytest.mark.parametrize('obs_mode,raster', [('state', 'ray'), ('pixels', 'ray'), ('pixels_dirty', 'ray'), ('state', 'alt'), ('pixels', 'alt'),
                                             ('pixels_dirty', 'alt')])
def test_batch_imagine_against_the_model(obs_mode, raster):
    """65 536 envs, 21x21, the mixed eight-menu table, auto_reset=False, phases spread by 40 random steps (+ reset_envs(done)).  A ~3 % mask with a random
    desired mask per env, then every env with its own mask: goal grid and agent, frames, the one_hot=True output and the stream afterwards of every
    selected env against the model; every buffer, state field and stream of every unselected env against its value before the call."""
    N, alt = 65536, raster == 'alt'
    kw = dict(size=(21, 21), max_steps=37)
    env_menu = (np.arange(N) % 8).astype(np.uint8)
    env, _, _ = make_env(N, obs_mode=obs_mode, seed=91, raster=raster, auto_reset=False, task_menus=_MENUS8, env_menu=env_menu, **kw)
    env.reset()
    env.set_state(step_num=(np.arange(N) % 31).astype(np.int32))     # (envs finish on every one of the 40 steps)
    _spread(env, 40, 3)
    rng = np.random.RandomState(17)
    for call in range(2):
        st0, (k0, p0), dev0 = env.get_state(), env.get_rng_states(), _device_side(env)
        if call == 0:
            mask = rng.rand(N) < 0.03
            desired = rng.randint(0, 512, N).astype(np.uint16)
            frames = env.imagine_obs(torch.as_tensor(mask, device=env.device), desired=desired)
        else:
            mask = np.ones(N, bool)
            desired = st0['desired']
            frames = env.imagine_obs()
        rows, rest = np.flatnonzero(mask), np.flatnonzero(~mask)
        assert call == 1 or 1500 < len(rows) < 2500
        if call == 0:
            on_start = (st0['agent_rc'][rows] == st0['init_agent_rc'][rows]).all(axis=1)
            goto = (desired[rows] >> M.T_GOTOHOUSE) & 1 == 1
            assert (goto & on_start).any() and (goto & ~on_start).any()      # both sides of the GoToHouse branch are in the sample
        g, a, k2, p2 = _model(st0, k0, p0, rows, desired)
        canary = frames[torch.as_tensor(rest[:64], device=env.device)].clone() if len(rest) else None
        _frames_equal(frames, rows, g, a, alt, 'imagine_obs frames')
        # the same call again from the same streams, for the states themselves (rows of unselected envs are not written: the scratch keeps them)
        env.set_rng_states(k0, p0)
        oh = env.imagine_obs(None if call else torch.as_tensor(mask, device=env.device), desired=None if call else desired, one_hot=True)
        for lo in range(0, len(rows), 8192):
            sl = slice(lo, lo + 8192)
            have = oh[torch.as_tensor(rows[sl], device=env.device)].cpu().numpy()
            want = np.stack([M.one_hot(g[j], a[j]) for j in range(lo, min(lo + 8192, len(rows)))])
            same('imagine_obs(one_hot=True)', rows[sl], have, want)
        if canary is not None:
            assert torch.equal(frames[torch.as_tensor(rest[:64], device=env.device)], canary)
        k1, p1 = env.get_rng_states()
        same('stream key after imagine_obs', rows, k1[rows], k2)
        same('stream position after imagine_obs', rows, p1[rows], p2)
        # nothing was committed: every env's state and buffers are as before; unselected envs' streams too
        _state_equal(env.get_state(), st0, slice(None))
        _rows_equal(_device_side(env), dev0, None, 'not committed: ')
        if len(rest):
            assert np.array_equal(k1[rest], k0[rest]) and np.array_equal(p1[rest], p0[rest])
    env.close()


@pytest.mark.parametrize('obs_mode,raster', [('pixels', 'ray'), ('pixels_dirty', 'alt'), ('state', 'ray')])
def test_commit_relabels_the_running_episode(obs_mode, raster):
    """commit=True with a desired mask per env on about half of 16 384 envs: desired_goal frames, goal_grid, desired_mask and hdr of the selected envs are the
    model's, everything else of every env is untouched; then 60 steps + reset_envs(done) equal the oracle with the new desired masks injected."""
    from oracle import OracleBatch
    N, T0, T1, alt = 16384, 40, 60, raster == 'alt'
    kw = dict(size=(21, 21), max_steps=37)
    env_menu = (np.arange(N) % 8).astype(np.uint8)
    env, keys, pos = make_env(N, obs_mode=obs_mode, seed=5, raster=raster, auto_reset=False, task_menus=_MENUS8, env_menu=env_menu, **kw)
    env.reset()
    acts0 = _spread(env, T0, 8)
    st0, (k0, p0), dev0 = env.get_state(), env.get_rng_states(), _device_side(env)
    rng = np.random.RandomState(23)
    mask = rng.rand(N) < 0.5
    desired = rng.randint(0, 512, N).astype(np.uint16)
    rows, rest = np.flatnonzero(mask), np.flatnonzero(~mask)
    env.imagine_obs(indices=rows, desired=desired, commit=True)
    g, a, k2, p2 = _model(st0, k0, p0, rows, desired)
    st1, (k1, p1), dev1 = env.get_state(), env.get_rng_states(), _device_side(env)
    same('goal_grid', rows, st1['goal_grid'][rows], g)
    same('goal_agent_rc', rows, st1['goal_agent_rc'][rows], a)
    same('desired', rows, st1['desired'][rows], desired[rows])
    same('desired_mask', rows, env.desired_mask.cpu().numpy().view(np.uint16)[rows], desired[rows])
    hdr = env.hdr.cpu().numpy().astype(np.int64)
    same('hdr bytes 6-7', rows, (hdr[:, 6] | (hdr[:, 7] << 8))[rows], desired[rows].astype(np.int64))
    same('stream key', rows, k1[rows], k2)
    same('stream position', rows, p1[rows], p2)
    oh = env.one_hot(which='goal')
    same("one_hot(which='goal')", rows[:4096], oh[torch.as_tensor(rows[:4096], device=env.device)].cpu().numpy(),
         np.stack([M.one_hot(g[j], a[j]) for j in range(4096)]))
    if obs_mode != 'state':
        _frames_equal(env._observation()['desired_goal'], rows, g, a, alt, 'desired_goal frames')
    # everything else: the selected rows apart from their goal / desired, the unselected rows entirely, the counters
    _state_equal(st1, st0, rows, skip=('goal_grid', 'goal_agent_rc', 'desired'))
    _state_equal(st1, st0, rest)
    assert np.array_equal(k1[rest], k0[rest]) and np.array_equal(p1[rest], p0[rest])
    _rows_equal(dev1, dev0, rest, 'unselected: ')
    hdr0 = dev0['hdr'].clone()
    hdr0[torch.as_tensor(rows, device=env.device), 6:8] = dev1['hdr'][torch.as_tensor(rows, device=env.device), 6:8]
    assert torch.equal(dev1['hdr'], hdr0)                    # (of a selected env's header only bytes 6-7 moved)
    for k in ('slot_pos', 'reward', 'done', 'achieved_mask', 'episode_length', 'episode_return', 'counters', 'observation', 'init_observation'):
        if k in dev0:
            assert torch.equal(dev1[k], dev0[k]), k
    # the oracle at the same point: the same history, then the new desired masks and the streams as imagine_obs left them
    okw = oracle_kw(kw, raster)
    ora = OracleBatch(N, rng_states=list(zip(keys, pos)), per_env_kwargs=[_MENUS8[int(m)] for m in env_menu], **okw)
    ora.reset()
    ora.rollout(acts0.astype(np.int8), nthreads=16)
    for i in rows:
        e = ora.envs[i]
        v = e.view()
        e._lib.cwo_set_state(e._h, v.grid, v.init_grid, v.agent_r, v.agent_c, v.hold, v.achieved, int(desired[i]), v.step_num)
        e.set_rng(k1[i], int(p1[i]))
    gen = torch.Generator(device='cuda').manual_seed(77)
    acts1 = torch.randint(0, 6, (T1, N), device='cuda', dtype=torch.uint8, generator=gen)
    rs = torch.empty((T1, N), dtype=torch.int32, device='cuda')
    ds = torch.empty((T1, N), dtype=torch.bool, device='cuda')
    for t in range(T1):
        _, r, dn, _ = env.step(acts1[t])
        rs[t], ds[t] = r, dn
        env.reset_envs(env.done)
    torch.cuda.synchronize()
    total, o_rew, o_done = ora.rollout(acts1.cpu().numpy().astype(np.int8), nthreads=16, record=True)
    same('reward of every step', 0, rs.cpu().numpy().T, o_rew.T)
    same('done of every step', 0, ds.cpu().numpy().T, o_done.astype(bool).T)
    assert int(o_done.sum()) >= N                            # (every env finished at least once on the way)
    st2, (k3, p3) = env.get_state(), env.get_rng_states()
    want = oracle_arrays(ora.envs, ['rng_key'])
    fresh = o_done.any(axis=0)                               # reset since the injection: the oracle knows the whole episode record again
    for k in st2:
        sel = fresh if k in ('init_agent_rc', 'goal_grid', 'goal_agent_rc') else slice(None)
        same('after 60 steps: ' + k, np.arange(N)[sel], st2[k][sel], want[k][sel])
    same('after 60 steps: rng_key', 0, k3, want['rng_key'])
    same('after 60 steps: rng_pos', 0, p3, want['rng_pos'])
    stale = rows[~fresh[rows]]                               # a relabelled env that never finished: its goal is still the committed one
    if len(stale):
        j = np.flatnonzero(~fresh[rows])
        same('a committed goal stays until the next reset', stale, st2['goal_grid'][stale], g[j])
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ (3) look-ahead engines
def test_look_ahead_engine_rewinds_and_agrees():
    """auto_reset=True (records kept): results and streams equal the auto_reset=False engine's from identical states, counters[0..3] untouched, the
    following 2 * max_steps steps equal the oracle, and the call is refused inside a capture."""
    from oracle import OracleBatch
    N, T0 = 4096, 6
    kw = dict(size=(21, 21), max_steps=20)
    keys, pos = np_states(N, 52000)
    a, _, _ = make_env(N, keys, pos, obs_mode='pixels_dirty', auto_reset=False, **kw)
    b, _, _ = make_env(N, keys, pos, obs_mode='pixels_dirty', auto_reset=True, **kw)
    assert a.tuner_state()['lookahead'] == 0 and b.tuner_state()['lookahead'] == 1
    a.reset()
    b.reset()
    gen = torch.Generator(device='cuda').manual_seed(4)
    acts0 = torch.randint(0, 4, (T0, N), device='cuda', dtype=torch.uint8, generator=gen)
    for t in range(T0):
        a.step(acts0[t])
        b.step(acts0[t])
        assert not bool(a.done.any()) and not bool(b.done.any())
    rng = np.random.RandomState(3)
    mask = rng.rand(N) < 0.4
    desired = rng.randint(0, 512, N).astype(np.uint16)
    st0, (k0, p0) = b.get_state(), b.get_rng_states()
    ka, pa = a.get_rng_states()
    assert np.array_equal(ka, k0) and np.array_equal(pa, p0)  # (the look-ahead engine reports its streams at the envs' logical position)
    c0 = b._counters_raw[:4].clone()
    fa = a.imagine_obs(mask, desired=desired, commit=True).clone()
    fb = b.imagine_obs(mask, desired=desired, commit=True).clone()
    rows = np.flatnonzero(mask)
    r_dev = torch.as_tensor(rows, device=a.device)
    assert torch.equal(fa[r_dev], fb[r_dev])
    sa, sb = a.get_state(), b.get_state()
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
    (ka, pa), (kb, pb) = a.get_rng_states(), b.get_rng_states()
    assert np.array_equal(ka, kb) and np.array_equal(pa, pb)
    assert torch.equal(a._observation()['desired_goal'], b._observation()['desired_goal'])
    assert torch.equal(b._counters_raw[:4], c0)
    g, ag, k2, p2 = _model(st0, k0, p0, rows, desired)
    same('goal_grid', rows, sb['goal_grid'][rows], g)
    same('stream key', rows, kb[rows], k2)
    same('stream position', rows, pb[rows], p2)
    # the oracle from here on: the same history, the new desired masks, the streams as the call left them
    ora = OracleBatch(N, rng_states=list(zip(keys, pos)), **kw)
    ora.reset()
    ora.rollout(acts0.cpu().numpy().astype(np.int8), nthreads=16)
    for i in rows:
        e = ora.envs[i]
        v = e.view()
        e._lib.cwo_set_state(e._h, v.grid, v.init_grid, v.agent_r, v.agent_c, v.hold, v.achieved, int(desired[i]), v.step_num)
        e.set_rng(kb[i], int(pb[i]))
    T1 = 2 * kw['max_steps']
    acts1 = torch.randint(0, 6, (T1, N), device='cuda', dtype=torch.uint8, generator=gen)
    rs = torch.empty((T1, N), dtype=torch.int32, device='cuda')
    ds = torch.empty((T1, N), dtype=torch.bool, device='cuda')
    for t in range(T1):
        _, r, dn, _ = b.step(acts1[t])
        rs[t], ds[t] = r, dn
    torch.cuda.synchronize()
    _, o_rew, o_done = ora.rollout(acts1.cpu().numpy().astype(np.int8), nthreads=16, record=True)
    same('reward of every step', 0, rs.cpu().numpy().T, o_rew.T)
    same('done of every step', 0, ds.cpu().numpy().T, o_done.astype(bool).T)
    assert o_done.any(axis=0).all()                          # every env was reset since: the oracle knows every record
    st2, (k3, p3) = b.get_state(), b.get_rng_states()
    want = oracle_arrays(ora.envs, ['rng_key', 'desired_goal'])
    for k in st2:
        same('after the steps: ' + k, 0, st2[k], want[k])
    same('rng_key', 0, k3, want['rng_key'])
    same('rng_pos', 0, p3, want['rng_pos'])
    same('desired_goal frames', 0, b._observation()['desired_goal'].cpu().numpy(), want['desired_goal'])
    # inside a capture the look-ahead engine refuses (it would have to rewind through the host); the refusal enqueues nothing
    from gym_craftingworld_amd._lib import CraftingWorldError
    scratch = torch.zeros(8, device='cuda')
    m_dev = torch.as_tensor(mask, device=b.device)
    b.synchronize()
    graph = torch.cuda.CUDAGraph()
    refused = None
    with torch.cuda.graph(graph):
        scratch.add_(1)
        try:
            b.imagine_obs(m_dev, commit=True)
        except CraftingWorldError as exc:
            refused = str(exc)
    assert refused is not None and '(-3)' in refused and 'cw_imagine_masked' in refused
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------------------------------------ (4) capture
def test_step_imagine_and_masked_reset_captured_into_one_graph():
    """on an engine without look-ahead records cw_step + cw_imagine_masked(commit) + cw_reset_masked go into one graph; three replays equal the eager sequence"""
    from gym_craftingworld_amd import CraftingWorldVecEnv
    N = 2048
    kw = dict(size=(6, 6), max_steps=8, obs_mode='state', auto_reset=False, seed=29)
    eager, graphed = CraftingWorldVecEnv(N, **kw), CraftingWorldVecEnv(N, **kw)
    eager.reset()
    graphed.reset()
    ring = torch.zeros((1, N), dtype=torch.uint8, device='cuda')
    mask_t = torch.zeros(N, dtype=torch.bool, device='cuda')
    des_t = torch.zeros(N, dtype=torch.int16, device='cuda')
    out_g = torch.zeros((N,) + graphed.frame_shape, dtype=torch.uint8, device='cuda')
    out_e = torch.zeros_like(out_g)
    graphed.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graphed.step_many(ring)
        graphed.imagine_obs(mask_t, desired=des_t, commit=True, out=out_g)
        graphed.reset_envs(graphed.done)
    assert int(graphed.counters[0]) == 0                     # (capturing ran nothing)
    gen = torch.Generator(device='cuda').manual_seed(6)
    for r_ in range(3):
        ring.copy_(torch.randint(0, 6, (1, N), device='cuda', dtype=torch.uint8, generator=gen))
        mask_t.copy_(torch.rand(N, device='cuda', generator=gen) < 0.3)
        des_t.copy_(torch.randint(0, 512, (N,), device='cuda', dtype=torch.int16, generator=gen))
        g.replay()
        eager.step(ring[0])
        eager.imagine_obs(mask_t.clone(), desired=des_t.clone(), commit=True, out=out_e)
        eager.reset_envs(eager.done)
        torch.cuda.synchronize()
        assert torch.equal(graphed.hdr, eager.hdr) and torch.equal(graphed.slot_pos, eager.slot_pos), r_
        assert torch.equal(out_g, out_e), r_
    sa, sb = graphed.get_state(), eager.get_state()
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
    (ka, pa), (kb, pb) = graphed.get_rng_states(), eager.get_rng_states()
    assert np.array_equal(ka, kb) and np.array_equal(pa, pb)
    assert torch.equal(graphed.counters, eager.counters) and int(eager.counters[0]) == 3 * N
    eager.close()
    graphed.close()


# ------------------------------------------------------------------------------------------------------------------------------ (5) sample_states
@pytest.mark.parametrize('pooled', [False, True])
def test_sample_states_against_the_model(pooled):
    """every env of a 65 536 batch: a masked call and a call for all, fresh (21x21) and pooled (8x8, three placements per env); the env's state is untouched
    but for its stream"""
    N = 65536
    kw = dict(size=(8, 8), max_steps=30, fixed_init_state=3) if pooled else dict(size=(21, 21), max_steps=30)
    env, _, _ = make_env(N, obs_mode='state', seed=12, auto_reset=False, **kw)
    env.reset()
    _spread(env, 5, 2)
    pool = env.fixed_states() if pooled else None
    S = kw['size'][0]
    rng = np.random.RandomState(9)
    for call in range(2):
        st0, (k0, p0), dev0 = env.get_state(), env.get_rng_states(), _device_side(env)
        mask = rng.rand(N) < 0.03 if call == 0 else np.ones(N, bool)
        before = env.sample_states().view(torch.int16).clone().view(torch.uint16) if call == 0 else None      # (a call for all first, so that the scratch rows hold known values)
        if call == 0:
            env.set_rng_states(k0, p0)
        cells = (env.sample_states(mask, pooled=pooled) if call == 0 else env.sample_states(pooled=pooled)).cpu().numpy()
        rows, rest = np.flatnonzero(mask), np.flatnonzero(~mask)
        want = np.empty((len(rows), 9), np.uint16)
        k2, p2 = np.empty((len(rows), 624), np.uint32), np.empty(len(rows), np.int32)
        rs = np.random.RandomState()
        for j, i in enumerate(rows):
            rs.set_state(('MT19937', k0[i], int(p0[i]), 0, 0.0))
            want[j] = M.generate_fixed_initial_state(pool[i], rs) if pooled else M.sample_state(S, rs)
            s = rs.get_state()
            k2[j], p2[j] = s[1], s[2]
        same('sample_states', rows, cells[rows], want)
        if call == 0:
            assert np.array_equal(cells[rest], before.cpu().numpy()[rest])   # rows of unselected envs are not written
        k1, p1 = env.get_rng_states()
        same('stream key', rows, k1[rows], k2)
        same('stream position', rows, p1[rows], p2)
        if len(rest):
            assert np.array_equal(k1[rest], k0[rest]) and np.array_equal(p1[rest], p0[rest])
        _state_equal(env.get_state(), st0, slice(None))
        _rows_equal(_device_side(env), dev0, None, 'sample_states: ')
    if not pooled:
        with pytest.raises(ValueError):
            env.sample_states(pooled=True)
        out = torch.zeros((N, 9), dtype=torch.int16, device='cuda')
        assert env._lib.cw_sample_state_masked(env._h, None, 1, C.c_void_p(out.data_ptr()), env._stream()) == -1      # CW_ERR_INVALID
        assert env._lib.cw_imagine_masked(env._h, None, None, 0, None, None, env._stream()) == -1                       # nothing to do
    env.close()


def test_calls_before_the_first_reset_are_refused():
    from gym_craftingworld_amd import CraftingWorldVecEnv
    from gym_craftingworld_amd._lib import CraftingWorldError
    env = CraftingWorldVecEnv(64, size=(5, 5), obs_mode='state', seed=1)
    with pytest.raises(CraftingWorldError, match=r'\(-3\)'):
        env.imagine_obs()
    with pytest.raises(CraftingWorldError, match=r'\(-3\)'):
        env.sample_states()
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ (6) shards
def test_multi_device_pass_throughs_equal_the_single_batch():
    from gym_craftingworld_amd import CraftingWorldVecEnv
    from gym_craftingworld_amd.adapters import MultiDeviceVecEnv
    N = 1000
    kw = dict(size=(7, 7), max_steps=25, obs_mode='pixels_dirty', auto_reset=False)
    one = CraftingWorldVecEnv(N, seed=40, **kw)
    two = MultiDeviceVecEnv(N, ['cuda:0', 'cuda:0'], seed=40, **kw)
    one.reset()
    two.reset()
    acts = torch.randint(0, 4, (5, N), device='cuda', dtype=torch.uint8, generator=torch.Generator(device='cuda').manual_seed(1))
    for t in range(5):
        one.step(acts[t])
        two.step(acts[t])
    two.synchronize()
    rng = np.random.RandomState(2)
    mask = rng.rand(N) < 0.5
    rows = rng.randint(0, 2, (N, 9))
    f1 = one.imagine_obs(mask, desired=rows, commit=True).clone()
    f2 = two.imagine_obs(mask, desired=rows, commit=True)
    c1 = one.sample_states(indices=np.flatnonzero(mask)).view(torch.int16).clone()
    c2 = two.sample_states(indices=np.flatnonzero(mask))
    two.synchronize()
    sel = torch.as_tensor(np.flatnonzero(mask), device='cuda')
    assert torch.equal(torch.cat(f2)[sel], f1[sel])
    assert torch.equal(torch.cat([c.view(torch.int16) for c in c2])[sel], c1[sel])
    s1 = one.get_state()
    s2 = [sh.get_state() for sh in two.shards]
    for k in s1:
        assert np.array_equal(s1[k], np.concatenate([s[k] for s in s2])), k
    k1, p1 = one.get_rng_states()
    k2 = np.concatenate([sh.get_rng_states()[0] for sh in two.shards])
    p2 = np.concatenate([sh.get_rng_states()[1] for sh in two.shards])
    assert np.array_equal(k1, k2) and np.array_equal(p1, p2)
    assert torch.equal(torch.cat([sh._observation()['desired_goal'] for sh in two.shards]), one._observation()['desired_goal'])
    one.close()
    two.close()
