"""GPU tier: cw_reset_masked_kernel, cw_imagine_masked_kernel and cw_sample_state_masked_kernel at every dealing width (epb = 4, 8, 16, 32, 64), with a
second round of the grid-stride loop, under the mask patterns that exercise the dealing (a full chunk beside an empty one, the last env, the last partial
chunk, 5 and 9 envs in a row, chunk edges, nothing, bytes other than 0 / 1, desired words with bits above the task list), at tiny batches and at the
grid sizes where the cell arithmetic of imagine / sample can go wrong (4x4: 7 free cells; 182x182 and 255x255: cells above 32 767).
Everything is bit-exact and EVERY selected env is compared: imagine and sample with the numpy model through masked_check.check_masked_call (itself tested
on the CPU, tests/test_masked_shapes_logic.py), resets with the CPU oracle through tests/oracle_replay.py.  The widths come from CW_TUNE_RESET_BLOCKS=1
(set before the engine is created: it is read once, at cw_create) and the card's CU count by the rule of DESIGN.md 5.1 (masked_check.masked_launch);
each test asserts the epb and chunk count it means to run.  No timing."""
import numpy as np
import pytest
import torch

import imagine_model as M
from engines import K5, n_cu
from masked_check import check_masked_call, masked_launch, model_imagine, spread, take, untouched
from oracle_replay import assert_counters, make_env, np_states, oracle_kw, replay_against_oracle, same, same_states

pytestmark = pytest.mark.gpu

# width -> (epb, N from most = n_cu workgroups, chunks); on 256 CUs: N = 509, 2 053, 4 099, 8 209, 16 411 and 20 011 (313 chunks on 256 workgroups)
WIDTHS = {'epb4': (4, lambda most: 2 * most - 3, lambda most: (2 * most) // 4),
          'epb8': (8, lambda most: 8 * most + 5, lambda most: most + 1),
          'epb16': (16, lambda most: 16 * most + 3, lambda most: most + 1),
          'epb32': (32, lambda most: 32 * most + 17, lambda most: most + 1),
          'epb64': (64, lambda most: 64 * most + 27, lambda most: most + 1),
          'round2': (64, lambda most: 64 * (most + most * 57 // 256 - 1) + 43, lambda most: most + most * 57 // 256)}
ALL_WIDTHS = list(WIDTHS)


def _width(width):
    """-> (N, epb, chunks) of a width case on this card, asserted against the launch rule"""
    most = n_cu()
    epb, n_of, chunks_of = WIDTHS[width]
    N, chunks = n_of(most), chunks_of(most)
    assert masked_launch(N, most, 1) == (epb, chunks, min(chunks, most)), (width, most, N, masked_launch(N, most, 1))
    assert N % 2 == 1 and N % epb != 0
    assert chunks > most if width == 'round2' else chunks <= most + 1
    return N, epb, chunks


def _engine(monkeypatch, N, blocks=1, seed=977, **kw):
    """-> (engine, keys, pos), created under CW_TUNE_RESET_BLOCKS=blocks (None: the default)"""
    with monkeypatch.context() as m:
        if blocks is not None:
            m.setenv('CW_TUNE_RESET_BLOCKS', str(blocks))
        return make_env(N, seed=seed, **kw)


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device='cuda')


def _desired(N):
    """every one of the 512 masks occurs (N >= 512), every 16th env desires nothing (the start state, no draw)"""
    d = ((np.arange(N) * 37 + 11) % 512).astype(np.uint16)
    d[::16] = 0
    return d


def _imagine_checked(env, mask, desired, commit=False, one_hot=True, frames=False, desired_dev=None, allow_empty=False):
    """imagine_obs(mask, desired, commit) into tensors of this test's own (filled with 7s), once per requested output from the same streams, each
    checked by check_masked_call against the snapshot before the first call.  mask: numpy bytes / bools or a device tensor handed over in place; desired:
    numpy words; desired_dev: the device tensor to hand over in its place."""
    before = take(env)
    mask_np = None if mask is None else (mask.cpu().numpy() if torch.is_tensor(mask) else np.asarray(mask))
    mask_t = mask if mask is None or torch.is_tensor(mask) else _dev(mask_np)
    des_arg = desired_dev if desired_dev is not None else desired
    alt = env.raster == 'alt'
    rows = None
    for n, oh in enumerate(([True] if one_hot else []) + ([False] if frames else [])):
        shape = (env.num_envs, env.size, env.size, 12) if oh else (env.num_envs,) + tuple(env.frame_shape)
        out = torch.full(shape, 7, dtype=torch.uint8, device='cuda')
        if n:
            env.set_rng_states(before['rng_key'], before['rng_pos'])
        got = env.imagine_obs(mask_t, desired=des_arg, commit=commit, one_hot=oh, out=out)
        assert got is out
        rows = check_masked_call('imagine', before, take(env), mask_np, desired=desired, commit=commit, alt=alt, allow_empty=allow_empty,
                                 out_before=np.full(shape, 7, np.uint8), n_task_list=len(env.task_list),
                                 **{'one_hot' if oh else 'frames': got.cpu().numpy()})
    return before, rows


def _sample_checked(env, mask, pooled=False, allow_empty=False):
    """sample_states(mask, pooled) checked against the model; the scratch rows of the unselected envs keep what the call before left there"""
    scratch = getattr(env, '_sample_cells', None)
    prev = np.zeros((env.num_envs, 9), np.uint16) if scratch is None else scratch.cpu().numpy().copy()
    before = take(env)
    mask_np = None if mask is None else (mask.cpu().numpy() if torch.is_tensor(mask) else np.asarray(mask))
    mask_t = mask if mask is None or torch.is_tensor(mask) else _dev(mask_np)
    cells = env.sample_states(mask_t, pooled=pooled).cpu().numpy()
    assert cells.dtype == np.uint16
    check_masked_call('sample', before, take(env), mask_np, cells=cells, out_before=prev, pool=env.fixed_states() if pooled else None,
                      allow_empty=allow_empty)
    return before, cells


def _phases(env, kw):
    phase = (np.arange(env.num_envs) % kw['max_steps']).astype(np.int32)
    env.set_state(step_num=phase)
    return phase


# ------------------------------------------------------------------------------------------------------------------------------ (a) the widths
@pytest.mark.parametrize('width', ALL_WIDTHS)
def test_imagine_at_every_width_against_the_model(monkeypatch, width):
    """5x5, state mode, auto_reset=False, phases spread by 8 random steps + reset_envs(done): a ~30 % mask, a desired word per env (all 512 values
    occur, every 16th nothing), goal states and frames from the same streams"""
    N, epb, chunks = _width(width)
    env, _, _ = _engine(monkeypatch, N, obs_mode='state', auto_reset=False, **K5)
    env.reset()
    _phases(env, K5)
    spread(env, 8, 3)
    mask = np.random.RandomState(epb + chunks).rand(N) < 0.3
    mask[N - 1] = True                                           # (the last, partial chunk holds a selected env)
    before, rows = _imagine_checked(env, mask, _desired(N), frames=True)
    assert 0.2 * N < len(rows) < 0.4 * N
    home = (before['state_agent_rc'][rows] == before['state_init_agent_rc'][rows]).all(axis=1)
    goto = (_desired(N)[rows] >> M.T_GOTOHOUSE) & 1 == 1
    assert (goto & home).any() and (goto & ~home).any()
    env.close()


@pytest.mark.parametrize('width,obs_mode,raster', [('epb8', 'pixels_dirty', 'alt'), ('epb32', 'pixels', 'ray')])
def test_committed_imagine_with_pixels_against_the_model(monkeypatch, width, obs_mode, raster):
    """commit=True in the pixel modes: the desired_goal frames, goal records, desired_mask and hdr bytes 6-7 of the selected rows are the model's, the
    unselected rows and every other frame array are untouched"""
    N, epb, chunks = _width(width)
    env, _, _ = _engine(monkeypatch, N, obs_mode=obs_mode, raster=raster, auto_reset=False, **K5)
    env.reset()
    _phases(env, K5)
    spread(env, 8, 4)
    mask = np.random.RandomState(chunks).rand(N) < 0.3
    _imagine_checked(env, mask, _desired(N), commit=True, frames=True)
    env.close()


@pytest.mark.parametrize('width', ALL_WIDTHS)
def test_sample_states_at_every_width_against_the_model(monkeypatch, width):
    """fresh placements (every env, then a ~30 % mask), then pooled ones (fixed_init_state=3)"""
    N, epb, chunks = _width(width)
    env, _, _ = _engine(monkeypatch, N, obs_mode='state', auto_reset=False, fixed_init_state=3, **K5)
    env.reset()
    spread(env, 3, 5)
    mask = np.random.RandomState(epb).rand(N) < 0.3
    _sample_checked(env, None)
    _sample_checked(env, mask)
    _, cells = _sample_checked(env, mask, pooled=True)
    pool = env.fixed_states()
    rows = np.flatnonzero(mask)
    assert all((pool[i] == cells[i]).all(axis=1).any() for i in rows[:64])         # (a pooled row is one of the env's three placements)
    env.close()


def _manual_reset_loop(env, acts):
    rs = torch.empty(acts.shape, dtype=torch.int32, device=acts.device)
    ds = torch.empty(acts.shape, dtype=torch.bool, device=acts.device)
    for t in range(acts.shape[0]):
        _, r, d, _ = env.step(acts[t])
        rs[t] = r
        ds[t] = d
        env.reset_envs(env.done)
    torch.cuda.synchronize()
    return rs.cpu().numpy(), ds.cpu().numpy()


@pytest.mark.parametrize('width,obs_mode', [(w, 'state') for w in ALL_WIDTHS] + [('round2', 'pixels_dirty')])
def test_manual_reset_at_every_width_equals_the_oracles_auto_reset(monkeypatch, width, obs_mode):
    """auto_reset=False + reset_envs(env.done) after each of 40 steps (max_steps 17, phases spread: envs finish on every step) == the oracle's auto-reset
    rollout: every reward and done, and state, episode counts, frames and RNG of every env at the end; the PAINT variant takes a second round too"""
    N, epb, chunks = _width(width)
    env, keys, pos = _engine(monkeypatch, N, obs_mode=obs_mode, auto_reset=False, **K5)
    env.reset()
    phase = _phases(env, K5)
    acts = torch.randint(0, 6, (40, N), device='cuda', dtype=torch.uint8, generator=torch.Generator(device='cuda').manual_seed(chunks))
    r_host, d_host = _manual_reset_loop(env, acts)
    per_step = d_host.sum(axis=1)
    assert per_step.min() > 0 and per_step.max() < N                            # (every mask a proper, non-empty subset)
    res = replay_against_oracle(env, keys, pos, oracle_kw(K5), acts.cpu().numpy(), r_host, d_host, phase=phase, frames=obs_mode != 'state')
    assert res['done_per_env'].min() >= 2
    assert_counters(env, N, 40, res)
    assert env.tuner_state()['lookahead'] == 0
    env.close()


@pytest.mark.parametrize('width', ['epb32', 'round2'])
def test_forced_resets_on_a_look_ahead_engine_at_two_widths(monkeypatch, width):
    """auto_reset=True: after every step a forced reset of a seeded ~10 % of the envs, in lock step with the oracle.  The first one finds every ring
    full (records taken over: counters[5] stands); after step 4 the same mask six times in a row runs the selected rings dry (the slow path)."""
    from oracle import OracleBatch
    N, epb, chunks = _width(width)
    kw, T = dict(size=(5, 5), max_steps=20), 10
    env, keys, pos = _engine(monkeypatch, N, obs_mode='state', **kw)
    ora = OracleBatch(N, rng_states=list(zip(keys, pos)), **kw)
    assert env.tuner_state()['lookahead'] == 1
    env.reset()
    ora.reset()
    rng = np.random.RandomState(chunks)
    acts = rng.randint(0, 6, (T, N)).astype(np.int8)
    dacts = torch.as_tensor(acts, device=env.device).to(torch.uint8)
    slow = lambda: int(env._counters_raw[5].item())            # noqa: E731
    res = dict(finished=0, successes=0)
    taken_over = ran_dry = 0
    for t in range(T):
        _, rew, done, _ = env.step(dacts[t])
        _, o_rew, o_done = ora.rollout(acts[t:t + 1], nthreads=16, record=True)
        same('reward of step %d' % t, 0, rew.cpu().numpy(), o_rew[0])
        same('done of step %d' % t, 0, done.cpu().numpy(), o_done[0].astype(bool))
        res['finished'] += int(o_done.sum())
        res['successes'] += int((o_rew == kw['max_steps']).sum())
        mask = rng.rand(N) < 0.1
        m_dev = torch.as_tensor(mask, device=env.device)
        for rep in range(6 if t == 4 else 1):
            s0 = slow()
            env.reset_envs(m_dev)
            for i in np.flatnonzero(mask):
                ora.envs[i]._lib.cwo_reset(ora.envs[i]._h)
            if t == 0:
                assert slow() == s0                              # every selected env took over a waiting record
                taken_over += int(mask.sum())
            ran_dry += slow() - s0
        if t in (0, 4, T - 1):
            same_states(env, ora, tag='step %d: ' % t)
    assert taken_over > 0 and ran_dry > 0, (taken_over, ran_dry)
    assert_counters(env, N, T, res)
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ (b) the mask patterns
PATTERNS = ['full_chunk_beside_an_empty_one', 'last_env', 'last_partial_chunk', 'five_in_a_chunk', 'nine_in_a_row', 'chunk_edges', 'all_zero', 'odd_bytes',
            'desired_high_bits']


def _pattern(name, N, epb, chunks):
    """-> the mask bytes (uint8).  Chunk c holds envs c * epb .. c * epb + epb - 1; the last chunk is partial."""
    m = np.zeros(N, np.uint8)
    rng = np.random.RandomState(len(name))
    if name == 'full_chunk_beside_an_empty_one':                 # (in the second-round case a chunk of the second round)
        c = chunks - 3
        m[c * epb:(c + 1) * epb] = 1
        assert m.sum() == epb and not m[(c + 1) * epb:].any()
    elif name == 'last_env':
        m[N - 1] = 1
    elif name == 'last_partial_chunk':
        m[N // epb * epb:] = 1
        assert 0 < m.sum() < epb
    elif name == 'five_in_a_chunk':                               # ranks 0..4 over four waves: one wave takes two envs in turn on the same LDS state
        m[2 * epb + 1:2 * epb + 6] = 1
    elif name == 'nine_in_a_row':                                 # ... three (of a chunk of 8 the run fills it and goes on into the next)
        m[5 * epb + 2:5 * epb + 11] = 1
        assert m.sum() == 9
    elif name == 'chunk_edges':
        m[[0, epb - 1, epb, epb + 1]] = 1
    elif name == 'odd_bytes':                                     # no 1 among them
        sel = rng.rand(N) < 0.2
        m[sel] = rng.choice(np.array([2, 0x80, 0xFF], np.uint8), int(sel.sum()))
        assert not (m == 1).any() and {2, 0x80, 0xFF} <= set(m.tolist())
    elif name == 'desired_high_bits':
        m[rng.rand(N) < 0.2] = 1
    return m


@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('width', ['epb8', 'round2'])
def test_mask_patterns_through_reset_imagine_and_sample(monkeypatch, width, pattern):
    """each pattern through reset_envs (against the oracle, the unselected rows byte for byte), imagine_obs(one_hot=True) and sample_states (against the
    model), the mask handed over in place as a device tensor: torch.bool, or torch.uint8 for the bytes other than 0 / 1"""
    from oracle import OracleBatch
    N, epb, chunks = _width(width)
    env, keys, pos = _engine(monkeypatch, N, obs_mode='state', auto_reset=False, **K5)
    ora = OracleBatch(N, rng_states=list(zip(keys, pos)), **K5)
    env.reset()
    ora.reset()
    ora.rollout(spread(env, 4, 6).astype(np.int8), nthreads=16)
    m = _pattern(pattern, N, epb, chunks)
    rows = np.flatnonzero(m)
    m_dev = _dev(m) if pattern == 'odd_bytes' else _dev(m != 0)
    assert m_dev.dtype == (torch.uint8 if pattern == 'odd_bytes' else torch.bool)
    # reset
    before = take(env)
    env.reset_envs(m_dev)
    after = take(env)
    untouched(before, after, m, 'reset_envs: ')
    assert np.array_equal(after['counters'], before['counters'])                  # (no look-ahead records: nothing is counted)
    for i in rows:
        ora.envs[i]._lib.cwo_reset(ora.envs[i]._h)
    same_states(env, ora, tag='after reset_envs: ')
    assert (after['state_step_num'][rows] == 0).all()
    assert np.array_equal(after['state_ep_no'][rows], before['state_ep_no'][rows] + (before['state_step_num'][rows] > 0))      # ray.py:200-201
    # imagine and sample
    empty = pattern == 'all_zero'
    desired = _desired(N)
    if pattern == 'desired_high_bits':                            # bits 9..15 on top of valid masks, 0xFFFF among them, as an int16 device tensor; committed
        hi = np.random.RandomState(8).randint(1, 128, N).astype(np.uint16) << 9
        desired = desired | hi
        desired[rows[::7]] = 0xFFFF
        d_dev = _dev(desired.view(np.int16))
        assert d_dev.dtype == torch.int16 and (desired[rows] >> 9).min() > 0
        _imagine_checked(env, m_dev, desired, commit=True, desired_dev=d_dev)
        got = take(env)
        same('committed desired_mask', rows, got['desired_mask'][rows], desired[rows] & 0x1FF)
        same('committed hdr bytes 6-7', rows, got['hdr'][rows, 6].astype(np.int64) | (got['hdr'][rows, 7].astype(np.int64) << 8), (desired[rows] & 0x1FF).astype(np.int64))
    else:
        _imagine_checked(env, m_dev, desired, allow_empty=empty)
    _sample_checked(env, m_dev, allow_empty=empty)
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ (c) tiny batches
@pytest.mark.parametrize('N', [1, 2, 3, 5, 63, 64, 65])
def test_tiny_and_boundary_batches(monkeypatch, N):
    """default tuning (epb = 4), 4x4: reset_envs(all ones) against reset() of a twin, one selected env through reset (oracle), imagine and sample (model),
    and every env through imagine (own masks, then desired given) and sample"""
    from oracle import OracleBatch
    assert masked_launch(N, n_cu())[0] == 4
    kw = dict(size=(4, 4), max_steps=9)
    env, keys, pos = _engine(monkeypatch, N, blocks=None, obs_mode='state', auto_reset=False, **kw)
    twin, _, _ = _engine(monkeypatch, N, blocks=None, obs_mode='state', auto_reset=False, **kw)
    ora = OracleBatch(N, rng_states=list(zip(keys, pos)), **kw)
    ora.reset()
    for e in (env, twin):
        e.reset()
        acts = spread(e, 3, 7, moves_only=True)
    ora.rollout(acts.astype(np.int8), nthreads=1)
    twin.reset()
    env.reset_envs(torch.ones(N, dtype=torch.uint8, device='cuda'))
    ora.reset()
    a, b = take(env), take(twin)
    for k in a:
        assert np.array_equal(a[k], b[k]), 'all-ones mask against reset(): ' + k
    same_states(env, ora, tag='all-ones mask: ')
    twin.close()
    ora.rollout(spread(env, 2, 8, moves_only=True).astype(np.int8), nthreads=1)
    one = np.zeros(N, np.uint8)
    one[N // 2] = 1
    m_dev = _dev(one != 0)
    before = take(env)
    env.reset_envs(m_dev)
    after = take(env)
    if N > 1:
        untouched(before, after, one, 'one env reset: ')
    ora.envs[N // 2]._lib.cwo_reset(ora.envs[N // 2]._h)
    same_states(env, ora, tag='one env reset: ')
    spread(env, 1, 9, moves_only=True)
    _imagine_checked(env, None, None)                            # every env, its own mask
    _imagine_checked(env, None, _desired(N) | 1)
    _sample_checked(env, None)
    _imagine_checked(env, m_dev, _desired(N) | 0x120)            # one env: GoToHouse and MoveSticks among its tasks
    _sample_checked(env, m_dev)
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ (d) grid size edges
MOVES = [(-1, 0), (0, 1), (1, 0), (0, -1)]                       # action ids 0..3: up, right, down, left
ROCK, TREE = 4, 5                                                # (walls for an agent that holds nothing)


def _a_move_that_moves(grid, rc):
    S = grid.shape[0]
    for a, (dr, dc) in enumerate(MOVES):
        r, c = int(rc[0]) + dr, int(rc[1]) + dc
        if 0 <= r < S and 0 <= c < S and grid[r, c] not in (ROCK, TREE):
            return a
    return 6


@pytest.mark.parametrize('obs_mode,raster', [('state', 'ray'), ('pixels', 'ray'), ('pixels', 'alt')])
def test_dense_grid_every_mask_on_both_sides_of_the_home_flag(obs_mode, raster):
    """4x4 (7 free cells of 16: kth_unoccupied and the draw ranges at their tightest), N = 2 048: the even envs take the no-op action 6 and stay on their
    start cell, every odd env takes a move that moves it (numpy states 95 008 + i: checked with the oracle on the CPU, none of them is walled in); the
    512 masks are dealt out by rank within each half, so every mask occurs exactly twice on either side of the home flag."""
    N = 2048
    keys, pos = np_states(N, 95008)
    env, _, _ = make_env(N, keys, pos, obs_mode=obs_mode, raster=raster, auto_reset=False, size=(4, 4), max_steps=30)
    env.reset()
    st = env.get_state()
    acts = np.array([6 if i % 2 == 0 else _a_move_that_moves(st['grid'][i], st['agent_rc'][i]) for i in range(N)], np.uint8)
    env.step(torch.as_tensor(acts, device='cuda'))
    st = env.get_state()
    home = (st['agent_rc'] == st['init_agent_rc']).all(axis=1)
    assert home[0::2].all() and int(home.sum()) >= N // 4 and int((~home).sum()) >= N // 4
    desired = np.zeros(N, np.uint16)
    desired[home] = np.arange(int(home.sum())) % 512
    desired[~home] = np.arange(int((~home).sum())) % 512
    assert np.bincount(desired[home], minlength=512).min() >= 2 and np.bincount(desired[~home], minlength=512).min() >= 2
    _imagine_checked(env, None, desired, one_hot=obs_mode == 'state', frames=obs_mode != 'state')
    _sample_checked(env, None)
    env.close()


@pytest.mark.parametrize('S,base', [(182, 61016), (255, 61000)])
def test_large_grids_cells_above_32767(S, base):
    """182x182 (33 124 cells) and 255x255 (65 025): uint16 cells that Python sees through int16 views, agent_cell_of's div_magic.  N = 8, state mode."""
    N = 8
    keys, pos = np_states(N, base)
    env, _, _ = make_env(N, keys, pos, obs_mode='state', auto_reset=False, size=(S, S), max_steps=30)
    env.reset()
    _, cells = _sample_checked(env, None)                        # (the numpy states were chosen on the CPU, with the model, for this)
    assert cells.dtype == np.uint16 and int((cells > 32767).sum()) >= 2
    _sample_checked(env, np.array([0, 1, 1, 0, 0, 1, 0, 1], bool))
    env.step(torch.as_tensor(np.array([0, 6, 1, 6, 2, 6, 3, 6], np.uint8), device='cuda'))
    bit = lambda *t: sum(1 << x for x in t)                      # noqa: E731
    desired = np.array([bit(M.T_MOVESTICKS), bit(M.T_MOVEAXE), bit(M.T_MOVEHAMMER), bit(M.T_GOTOHOUSE), 0x1FF, 0x1FF,
                        bit(M.T_GOTOHOUSE, M.T_MOVESTICKS, M.T_MOVEAXE, M.T_MOVEHAMMER), bit(M.T_GOTOHOUSE, M.T_BUILDHOUSE, M.T_CHOPTREE)], np.uint16)
    before, rows = _imagine_checked(env, None, desired, commit=True)
    home = (before['state_agent_rc'] == before['state_init_agent_rc']).all(axis=1)
    assert home.any() and (~home).any()
    st = env.get_state()
    g, a, _, _ = model_imagine({k[6:]: v for k, v in before.items() if k.startswith('state_')}, before['rng_key'], before['rng_pos'], rows, desired)
    same('goal_grid', rows, st['goal_grid'], g)
    same('goal_agent_rc', rows, st['goal_agent_rc'], a)
    same("one_hot(which='goal')", rows, env.one_hot(which='goal').cpu().numpy(), np.stack([M.one_hot(g[j], a[j]) for j in range(N)]))
    moved = np.concatenate([np.flatnonzero(g[j].reshape(-1) == c) for j in range(N) for c in (M.STICKS, M.AXE, M.HAMMER)])
    assert S < 255 or int(moved.max()) > 32767                   # (255x255: a moved object lands in the upper half of the cells)
    env.close()


def test_calls_that_must_leave_the_streams_alone():
    """fixed_init_state=1, 8x8: sample_states(pooled=True) returns the one pool row and draws nothing (randint(1)); imagine_obs(desired=zeros) returns
    the start state and draws nothing; every stream's key and position stay exactly as they were"""
    N = 777
    env, _, _ = make_env(N, seed=5, obs_mode='state', auto_reset=False, size=(8, 8), max_steps=30, fixed_init_state=1)
    env.reset()
    spread(env, 3, 1)
    k0, p0 = env.get_rng_states()
    mask = np.random.RandomState(1).rand(N) < 0.5
    for m in (None, mask):
        _, cells = _sample_checked(env, m, pooled=True)
        rows = np.arange(N) if m is None else np.flatnonzero(m)
        assert np.array_equal(cells[rows], env.fixed_states()[rows, 0])
        before, _ = _imagine_checked(env, m, np.zeros(N, np.uint16), frames=True)
        k1, p1 = env.get_rng_states()
        assert np.array_equal(k1, k0) and np.array_equal(p1, p0)
    oh = env.imagine_obs(desired=np.zeros(N, np.uint16), one_hot=True).cpu().numpy()
    same('nothing desired: the start state', 0, oh, env.one_hot(which='init').cpu().numpy())
    env.close()
