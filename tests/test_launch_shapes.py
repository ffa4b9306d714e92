"""GPU tests: the launch shapes the defaults never give a full-size batch, every env against the CPU oracle (tests/oracle_replay.py).
  (1) cw_rollout at every width cw_envs_per_wave gives it (64 / 32 / 16 / 8 envs per wave from N alone), with its segments (a refill ahead of each) at
      their default length, forced short (7: T not a multiple; 1) and off (CW_TUNE_ROLLOUT_SEGMENT=0: one launch), and rings of look-ahead records
      running dry inside a launch; each also against a twin of the same batch stepped with step().
  (2) the shapes only a CW_TUNE_* variable reaches (every value inside its documented range): the step kernel at 8 / 16 / 32 envs per wave
      in all three of its obs modes, the reset / refill / pool kernels with 1 and 16 workgroups per CU, the refill period forced to 1 and to 500 steps,
      the gather painter on 8x8 and 9x9 frames and turned off for 4x4 and 6x6, the small-frame sweep on 21x21 frames, at 1 and 8 workgroups per CU
      and turned off.
Each variable is set before the engine is created (it is read once, at cw_create), and compared with the oracle, never with another configuration."""
import numpy as np
import pytest
import torch

from oracle_replay import assert_counters, make_env, record_steps, replay_against_oracle

pytestmark = pytest.mark.gpu

EARLY_END = dict(size=(8, 8), max_steps=300, reward_style='subset', selected_tasks=['EatBread'], number_of_tasks=1)   # (as the early-end step test)


def _engine(monkeypatch, N, kw, tune=None, **mode):
    """-> (engine, keys, pos): created under the CW_TUNE_* variables `tune`, with the RNG states its oracle starts from"""
    with monkeypatch.context() as m:
        for k, v in (tune or {}).items():
            m.setenv(k, str(v))
        return make_env(N, seed=4242, **mode, **kw)


def _actions(T, N, seed, hi=6):
    return torch.randint(0, hi, (T, N), device='cuda', dtype=torch.uint8, generator=torch.Generator(device='cuda').manual_seed(seed))


def _phase(N, kw):
    return (np.arange(N) % (kw['max_steps'] - 1)).astype(np.int32)


# ------------------------------------------------------------------ (1) rollout


def _rollout_vs_oracle_and_stepping(monkeypatch, N, kw, T, phase, walker, segment=None):
    """one engine runs rollout(record=True), a twin of the same batch T x step(); both against each other, the rollout against the oracle.
    -> the rollout engine's counters"""
    tune = {} if segment is None else {'CW_TUNE_ROLLOUT_SEGMENT': segment}
    rolled, keys, pos = _engine(monkeypatch, N, kw, tune, obs_mode='state')
    stepped = _engine(monkeypatch, N, kw, keys=keys, pos=pos, obs_mode='state')[0]
    ph = _phase(N, kw) if phase else None
    for e in (rolled, stepped):
        e.reset()
        if phase:
            e.set_state(step_num=ph)
    acts = _actions(T, N, 31, 4 if walker else 6)
    rew, don = rolled.rollout(acts, record=True)
    rs = torch.empty((T, N), dtype=torch.int32, device='cuda')
    ds = torch.empty((T, N), dtype=torch.bool, device='cuda')
    for t in range(T):
        _, r, d, _ = stepped.step(acts[t])
        rs[t] = r
        ds[t] = d
    torch.cuda.synchronize()
    assert torch.equal(rew, rs) and torch.equal(don, ds)
    ever = ds.any(dim=0)
    assert torch.equal(stepped.episode_length[ever], rolled.episode_length[ever]) and torch.equal(stepped.episode_return[ever], rolled.episode_return[ever])
    assert torch.equal(stepped.reward, rolled.reward) and torch.equal(stepped.done, rolled.done) and torch.equal(stepped.achieved_mask, rolled.achieved_mask)
    assert torch.equal(stepped.counters, rolled.counters)
    res = replay_against_oracle(rolled, keys, pos, kw, acts.cpu().numpy(), rew.cpu().numpy(), don.cpu().numpy(), phase=ph)
    c = assert_counters(rolled, N, T, res)
    assert res['finished'] >= N
    stepped.close()
    rolled.close()
    return c, res


@pytest.mark.parametrize('N,T,segment', [(40009, 200, None), (20011, 200, None), (4099, 100, 7), (4099, 100, 1)],
                         ids=['width32_40009', 'width16_20011', 'segments_of_7', 'segments_of_1'])
def test_rollout_at_every_width_and_segment_length_against_the_oracle(monkeypatch, N, T, segment):
    """cw_rollout_kernel at 32 and 16 envs per wave (the last wave partly filled) with its default segments (64 steps), and at 8 with segments of 7
    (T not a multiple of it: the actions / rewards offsets of a short last segment) and of 1 (a refill ahead of every step); 9x9, max_steps 17,
    phases spread: envs finish on every step"""
    _rollout_vs_oracle_and_stepping(monkeypatch, N, dict(size=(9, 9), max_steps=17), T, True, False, segment)


def test_rollout_headline_shape_against_the_oracle(monkeypatch):
    """the README's state-only figure's shape: 65 536 envs (64 per wave), 21x21, max_steps 300, phases spread, 600 steps = two segments of 300
    with a refill between them"""
    _rollout_vs_oracle_and_stepping(monkeypatch, 65536, dict(size=(21, 21), max_steps=300), 600, True, False)


def test_rollout_whose_rings_run_dry_segmented_and_in_one_launch_against_the_oracle(monkeypatch):
    """episodes that end early (the early-end step test's batch: a walker on 8x8 grids, the one task EatBread) through cw_rollout at 64 envs per wave:
    envs finish several times inside one launch, their rings of look-ahead records run dry and the rollout kernel resets them the slow way.  With
    the default segments (300 steps) and in one launch of 450 steps, which refills less and so resets more of them the slow way"""
    c_seg, res = _rollout_vs_oracle_and_stepping(monkeypatch, 65536, EARLY_END, 450, False, True)
    assert res['finished'] > 2 * 65536
    assert int(c_seg[5]) > 0                                                 # (some rings ran dry inside a launch)
    c_one, _ = _rollout_vs_oracle_and_stepping(monkeypatch, 65536, EARLY_END, 450, False, True, segment=0)
    assert int(c_one[5]) > int(c_seg[5]), (int(c_one[5]), int(c_seg[5]))


# ------------------------------------------------------------------ (2) tuning variables


def _steps_vs_oracle(monkeypatch, N, kw, obs_mode, T, tune=None, keep_terminal_obs=False, phase=True, fixed=False):
    """T steps of random actions with episodes ending on every step (phases spread), every reward and done, and at the end the frames (pixel
    modes; terminal_observation with keep_terminal_obs), the state and the RNG state of every env against the oracle.  -> (engine, counters)"""
    env, keys, pos = _engine(monkeypatch, N, kw, tune, obs_mode=obs_mode, keep_terminal_obs=keep_terminal_obs)
    assert fixed == bool(kw.get('fixed_init_state'))                          # (make_env has redrawn the pool from the states the oracle gets)
    env.reset()
    ph = _phase(N, kw) if phase else None
    if phase:
        env.set_state(step_num=ph)
    acts = _actions(T, N, 17)
    rs, ds = record_steps(env, acts)
    res = replay_against_oracle(env, keys, pos, kw, acts.cpu().numpy(), rs, ds, phase=ph,
                                frames=obs_mode != 'state', terminal=keep_terminal_obs, pools=fixed)
    c = assert_counters(env, N, T, res)
    assert res['finished'] >= N
    return env, c


K8 = dict(size=(8, 8), max_steps=17)


@pytest.mark.parametrize('epw,N,obs_mode', [(8, 65536, 'state'), (8, 65509, 'pixels_dirty'), (8, 65536, 'pixels'),
                                            (16, 65509, 'state'), (16, 65536, 'pixels_dirty'), (16, 65509, 'pixels'),
                                            (32, 65536, 'state'), (32, 65509, 'pixels_dirty'), (32, 65536, 'pixels')])
def test_step_kernel_forced_width_against_the_oracle(monkeypatch, epw, N, obs_mode):
    """CW_TUNE_STEP_ENVS_PER_WAVE 8 / 16 / 32 on full-size batches (the defaults give them 64): cw_step_fused_kernel's state-only, dirty-cell
    and full-frame variants (the last two with keep_terminal_obs: the workgroup's queue of paint jobs holds the terminal frames too)"""
    env, _ = _steps_vs_oracle(monkeypatch, N, K8, obs_mode, 40, {'CW_TUNE_STEP_ENVS_PER_WAVE': epw}, keep_terminal_obs=obs_mode != 'state')
    env.close()


@pytest.mark.parametrize('N', [20011, 40009])
def test_step_kernel_default_widths_16_and_32_against_the_oracle(monkeypatch, N):
    """the batch sizes for which the defaults pick 16 and 32 envs per wave, dirty-cell frames with keep_terminal_obs, against the oracle (not only
    against the full-frame engine, which runs the same width)"""
    env, _ = _steps_vs_oracle(monkeypatch, N, K8, 'pixels_dirty', 40, keep_terminal_obs=True)
    env.close()


@pytest.mark.parametrize('blocks', [1, 16])
def test_reset_refill_and_pool_kernels_at_either_end_of_reset_blocks(monkeypatch, blocks):
    """CW_TUNE_RESET_BLOCKS 1 and 16: the reset, look-ahead refill and fixed_init_state pool kernels with 1 and 16 workgroups per CU; the pools
    (cw_get_fixed_states) against the oracle's (cwo_get_fixed_states) as well"""
    env, _ = _steps_vs_oracle(monkeypatch, 65536, dict(K8, fixed_init_state=5), 'pixels', 40, {'CW_TUNE_RESET_BLOCKS': blocks}, fixed=True)
    env.close()


@pytest.mark.parametrize('period', [1, 500])
def test_forced_refill_period_against_the_oracle(monkeypatch, period):
    """CW_TUNE_LA_PERIOD 1: a refill ahead of every step, so an env (which finishes at most once a step) always finds a record -- no slow reset.
    500: the one refill of 200 steps is the first one; an env finishes ~12 times on its way and its ring holds 4 records -- the rest (~8 per env) are
    reset the slow way"""
    N = 65536
    env, c = _steps_vs_oracle(monkeypatch, N, dict(size=(9, 9), max_steps=17), 'state', 200, {'CW_TUNE_LA_PERIOD': period})
    if period == 1:
        assert int(c[5]) == 0, int(c[5])
    else:
        assert int(c[5]) >= 5 * N, int(c[5])
    env.close()


@pytest.mark.parametrize('gmax,N,size', [(8, 40000, 8), (9, 30011, 9)])
def test_gather_painter_on_8x8_and_9x9_frames(monkeypatch, gmax, N, size):
    """CW_TUNE_GATHER_MAX_SIZE 8 / 9: the gather painter on 3.0 and 3.8 KiB frames (9x9: rows of 108 bytes straddle its 16-byte chunks)"""
    env, _ = _steps_vs_oracle(monkeypatch, N, dict(size=(size, size), max_steps=17), 'pixels', 40, {'CW_TUNE_GATHER_MAX_SIZE': gmax})
    assert env.render_kernel_name() == 'cw_render_gather_kernel'
    env.close()


@pytest.mark.parametrize('size', [4, 6])
def test_gather_painter_off_for_the_smallest_frames(monkeypatch, size):
    """CW_TUNE_GATHER_MAX_SIZE 0: 4x4 and 6x6 Ray frames, which go to the gather painter by default, through the piece sweep"""
    env, _ = _steps_vs_oracle(monkeypatch, 10007, dict(size=(size, size), max_steps=17), 'pixels', 40, {'CW_TUNE_GATHER_MAX_SIZE': 0})
    assert env.render_kernel_name() == 'cw_render_pieces_kernel'
    env.close()


@pytest.mark.parametrize('N,size,tune', [(8192, 21, {'CW_TUNE_SMALL_FRAME_BYTES': 1048576}),
                                         (65536, 5, {'CW_TUNE_SMALL_BLOCKS': 1}), (65536, 5, {'CW_TUNE_SMALL_BLOCKS': 8}),
                                         (65536, 5, {'CW_TUNE_SMALL_FRAME_BYTES': 0, 'CW_TUNE_GATHER': 0})],
                         ids=['21x21_as_small_frames', 'small_blocks_1', 'small_blocks_8', 'no_small_frames_no_gather'])
def test_small_frame_shapes_against_the_oracle(monkeypatch, N, size, tune):
    """CW_TUNE_SMALL_FRAME_BYTES 1 MiB: 21x21 frames (21 KiB) swept with 4 workgroups per CU (8 192 envs: 173 MB a sweep, under the 320-MB launch
    limit); CW_TUNE_SMALL_BLOCKS 1 and 8: the gather painter at either end; CW_TUNE_SMALL_FRAME_BYTES 0 with the gather painter off: 5x5 frames through
    the one-workgroup piece sweep"""
    env, _ = _steps_vs_oracle(monkeypatch, N, dict(size=(size, size), max_steps=17), 'pixels', 40, tune)
    if tune.get('CW_TUNE_GATHER') == 0:
        assert env.render_kernel_name() == 'cw_render_pieces_kernel'
    elif size == 5:
        assert env.render_kernel_name() == 'cw_render_gather_kernel'
    env.close()
