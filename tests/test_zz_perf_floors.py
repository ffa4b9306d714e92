"""GPU tier, collected LAST (the file name sorts after every other test file): everything whose verdict depends on the BOX -- rates, roofline
fractions, what the sweep clock's guard did, how long a host call took -- and the shape of bench.py's JSON line.  tests/test_hip_parity.py and
tests/test_facade_parity.py hold no such assertion: under `pytest -x` a throttled or busy box can only lose rows of THIS file, never hide an
oracle / fixture test behind a timing failure.  Where a test here also compares frames (the guard moving the clock must not change a pixel), the
pure bit-exact half of it lives in test_hip_parity.py too (test_frames_do_not_depend_on_the_sweeps_clock)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.gpu
def test_clock_guard_slows_a_saturated_sweep_down(monkeypatch):
    """The sweep's clock sets the rate at which a launch writes; its guard (cw_engine.cpp: sweep_guard_tick) holds every 64th sweep against its
    schedule and lowers the rate when three samples in a row are more than 6 % late (and raises it again only after 64 samples on time).  Started at 9 TB/s -- more than the memory system takes --
    the guard must have stepped the rate down within 2 000 steps; at the default rate it must stay within a notch; the frames are the dirty-cell
    engine's either way."""
    from gym_craftingworld_amd import CraftingWorldVecEnv
    N, kw = 65536, dict(size=(21, 21), max_steps=300, seed=3)
    acts = torch.randint(0, 6, (64, N), device='cuda', dtype=torch.uint8, generator=torch.Generator(device='cuda').manual_seed(2))
    dirty = CraftingWorldVecEnv(N, obs_mode='pixels_dirty', **kw)
    dirty.reset()
    for rate, T in (('9.0', 2000), (None, 1000)):
        if rate:
            monkeypatch.setenv('CW_TUNE_RATE_TBS', rate)
        e = CraftingWorldVecEnv(N, obs_mode='pixels', **kw)
        monkeypatch.delenv('CW_TUNE_RATE_TBS', raising=False)
        t0 = e.tuner_state()
        p0 = t0['period16']
        assert 0 < p0 < t0['period16_head'] < t0['period16_busy'], t0        # (a launch's head runs a notch slower, two after a busy step)
        e.reset()
        for t in range(T):                                   # (alone on the card: the guard times this engine's sweeps)
            e.step_async(acts[t % 64])
            if t % 250 == 249:
                torch.cuda.synchronize()
        ts = e.tuner_state()
        if rate:
            assert ts['guard_slowdowns'] >= 1 and ts['period16'] > p0 > 0, ts
            for t in range(T):
                dirty.step_async(acts[t % 64])
            for k in ('observation', 'desired_goal', 'init_observation'):
                assert torch.equal(e._observation()[k], dirty._observation()[k]), k
        else:
            # (at the edge one launch in ten is late, and a box in a worse state than at cw_create does not hold 7.7 TB/s: a notch or two, no more)
            assert ts['guard_slowdowns'] <= 2 and 0.96 * p0 <= ts['period16'] <= 1.07 * p0, ts
        e.close()
    dirty.close()


@pytest.mark.gpu
def test_clock_guard_probes_find_a_faster_clock_that_pays(monkeypatch):
    """Round 4's guard only ever lowered the rate; an engine created in a bad moment kept a clock under what the card takes for the rest of its life.  Round 5:
    after enough samples on time at the best rate known the guard tries one notch more and keeps it only if the sweeps get SHORTER (sweep_guard_tick).
    Started at 6.8 TB/s (617 ns) the clock must have climbed within 30 000 steps (three or four notches on every box so far; one is the test's floor: how far it
    pays is the card's state), never beyond the write path's edge (7.7 TB/s), with one slowdown counted at most; the frames are the dirty-cell engine's all the way."""
    from gym_craftingworld_amd import CraftingWorldVecEnv
    N, kw = 65536, dict(size=(21, 21), max_steps=300, seed=3)
    acts = torch.randint(0, 6, (64, N), device='cuda', dtype=torch.uint8, generator=torch.Generator(device='cuda').manual_seed(2))
    monkeypatch.setenv('CW_TUNE_RATE_TBS', '6.8')
    e = CraftingWorldVecEnv(N, obs_mode='pixels', **kw)
    monkeypatch.delenv('CW_TUNE_RATE_TBS')
    dirty = CraftingWorldVecEnv(N, obs_mode='pixels_dirty', **kw)
    e.reset(); dirty.reset()
    p0 = e.tuner_state()['period16']
    assert 980 <= p0 <= 995                               # (617 ns in 1/16 ticks of 10 ns)
    seen = []
    for t in range(30000):                                 # (alone on the card: another engine's steps between its sweeps are a disturbance the guard gives way to)
        e.step_async(acts[t % 64])
        if t % 3000 == 2999:
            torch.cuda.synchronize()
            seen.append(e.tuner_state()['period16'])
    for t in range(30000):
        dirty.step_async(acts[t % 64])
    for k in ('observation', 'desired_goal', 'init_observation'):
        assert torch.equal(e._observation()[k], dirty._observation()[k]), k
    assert torch.equal(e.counters, dirty.counters)
    ts = e.tuner_state()
    print('clock by 3000 steps:', seen, ts)
    assert ts['period16'] <= p0 - 20, (seen, ts)           # a notch and more (6.8 -> 7.0 TB/s: 987 -> 959; measured 6.8 -> 7.4 / 7.6: 907 / 883)
    assert ts['period16'] >= 865 and ts['guard_slowdowns'] <= 1, (seen, ts)      # (7.7 TB/s is 872; a probe undone is not a slowdown)
    assert all(b <= a + 30 for a, b in zip(seen, seen[1:])), seen                # (it climbs; a probe that does not pay is one notch -- ~25 units -- back)
    e.close(); dirty.close()


def test_bench_self_launched_two_ranks_share_the_gpu():
    """`python bench.py --gpus 2` started plainly (no torchrun): the parent starts two fresh ranks before touching HIP, both ranks
    run their env shard on this one GPU (--rehearse-on-one-gpu; gloo carries the timing barrier), rank 0's single JSON line comes
    back through the parent with n_gpus 2 and the whole-job rate.  Three processes use the GPU at most (two ranks + this test)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT')}
    # (rank 1 sleeps 30 ms on the host between its last launch and the closing barrier: a late rank at the barrier must not show in `value`)
    p = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '2', '--rehearse-on-one-gpu', '--dist-backend', 'gloo',
                        '--full', '--quick', '--steps', '12', '--warmup', '3', '--envs-per-gpu', '4096', '--max-steps', '20', '--inject-sleep-ms', '30',
                        '--inject-sleep-rank', '1'],
                       env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.strip().splitlines() if l.startswith('{')]
    assert len(lines) == 1, p.stdout
    d = json.loads(lines[0])
    assert d['n_gpus'] == 2 and d['steps'] == 12 and d['warmup'] == 3 and d['scaling'] == 'weak' and d['dist_backend'] == 'gloo'
    assert d['config']['envs_per_gpu'] == 4096 and d['value'] > 0
    assert abs(d['value'] - 2 * 4096 * 12 / (d['ms_per_step'] * 12e-3)) < 1e-6 * d['value']      # whole-job rate over both ranks
    # multi-rank regions are timed ON THE DEVICE (two events inside the barrier bracket): the 30 ms rank 1 spent asleep before the closing barrier are in
    # value_wall (the wall clock around the bracket, max over ranks) and nowhere in value
    assert abs(d['value_wall'] - 2 * 4096 * 12 / (d['ms_per_step_wall'] * 12e-3)) < 1e-6 * d['value_wall'] and 'DEVICE' in d['timing']
    assert d['ms_per_step_wall'] * 12 >= 30.0 > d['ms_per_step'] * 12, (d['ms_per_step_wall'], d['ms_per_step'])
    assert d['per_rank_ms_per_step_wall'][1] * 12 >= 30.0 and max(d['per_rank_ms_per_step']) * 12 < 30.0
    assert abs(max(d['per_rank_ms_per_step']) - d['ms_per_step']) < 1e-9
    # every rank explains itself on rank 0's line: its shard, its clock and guard, its sweep time against the roof, its NUMA binding (or why not)
    pr = d['per_rank']
    assert [r['rank'] for r in pr] == [0, 1] and [r['envs'] for r in pr] == [[0, 4096], [4096, 8192]]
    assert all(r['tuner']['guard_slowdowns'] in (-1, 0) and 'period16' in r['tuner'] for r in pr)
    assert all(0 < r['roofline_frac'] < 1 and r['sweep_ms'] > 0 for r in pr) and d['per_rank_roofline_frac'] == [r['roofline_frac'] for r in pr]
    assert all(r['barrier_ms'] > 0 and r['region_ms_wall'] >= r['region_ms_device'] > 0 for r in pr)
    assert all('skipped' in r['numa'] and 'rehearsal' in r['numa']['skipped'] for r in pr) and len(d['per_rank_tuner']) == 2
    assert d['policy_in_loop'] is None                   # (--quick)


@pytest.mark.gpu
def test_bench_json_line_carries_the_contract():
    """One small `python bench.py --full` run on this GPU: exactly one JSON line with the contract's keys, the roofline object (dominant kernel
    by the name a rocprofv3 trace lists it under, HIP-event launch times, average and median), the CPU baseline (kind "port", a described
    sample, like for like with the headline), the repeats and the metric window."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT')}
    p = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--full', '--steps', '40', '--warmup', '5', '--envs-per-gpu', '8192',
                        '--max-steps', '20', '--cpu-seconds', '0.5', '--no-other-modes', '--no-single-env'],
                       env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.strip().splitlines() if l.startswith('{')]
    assert len(lines) == 1 and p.stdout.strip().splitlines()[-1] == lines[0], p.stdout      # one JSON line, the LAST line of stdout
    d = json.loads(lines[0])
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline', 'dtype',
              'data', 'config', 'roofline', 'cpu_baseline', 'warmup_total', 'per_rank_ms_per_step', 'metric_window_desync'):
        assert k in d, k
    assert d['warmup_total'] == d['warmup'] + d['prewarm_steps'] and len(d['per_rank_ms_per_step']) == 1
    assert abs(d['per_rank_ms_per_step'][0] - d['ms_per_step']) < 1e-9
    wd = d['metric_window_desync']
    assert wd['steps'] == 40 and wd['value'] > 0 and 0 < wd['roofline']['frac'] < 1 and wd['resets_per_step'] > 8192 / 20 * 0.8
    assert 'traffic_source' in d['roofline']
    assert d['n_gpus'] == 1 and d['steps'] == 40 and d['warmup'] == 5 and d['higher_is_better'] is True and d['scaling'] == 'weak'
    assert d['vs_baseline'] is None and d['dtype'] == 'u8' and d['unit'] == 'env-steps/s' and 'workload' in d['config']
    assert abs(d['value'] - 8192 * 40 / (d['ms_per_step'] * 40e-3)) < 1e-6 * d['value']
    r = d['roofline']
    assert r['bound'] == 'hbm' and r['unit'] == 'GB/s' and r['peak'] == 8000.0 and 'traffic' in r
    assert r['kernel'] == 'cw_render_pieces_kernel' and r['kernel_in_trace'] == 'cw_render_pieces_kernel<0, 2>'
    assert r['avg_launch_ms'] > 0 and r['median_launch_ms'] > 0 and r['launch_ms_min_max'][0] <= r['median_launch_ms'] <= r['launch_ms_min_max'][1]
    assert abs(r['frac'] - r['achieved'] / r['peak']) < 1e-9 and 0 < r['frac'] < 1 and 0 < r['frac_at_median_launch'] < 1
    assert abs(r['achieved'] - r['algorithmic_bytes_per_launch'] / (r['avg_launch_ms'] * 1e-3) / 1e9) < 1e-6 * r['achieved']
    c = d['cpu_baseline']
    assert c['kind'] == 'port' and c['cores'] >= 1 and c['value'] > 0 and c['unit'] == 'env-steps/s' and isinstance(c['sample'], str)
    assert d['repeats']['n'] == 3 and d['repeats']['value'][0] == d['value']
    assert d['metric_window']['steps'] == 40 and d['metric_window']['value'] > 0 and len(d['metric_window']['slowest_step_ms']) == 2
    # round 5: the whole step against the roof; the engine with a consumer between two steps; the CPU baseline beside a GPU soak; per-rank blocks
    assert 0 < r['step_frac'] < r['frac'] and 0 < r['step_frac_metric_window'] < 1 and 0 < r['step_frac_metric_window_desync'] < 1
    assert abs(r['step_frac'] - r['step_algorithmic_bytes'] / (d['ms_per_step'] * 1e-3) / 1e9 / 8000.0) < 1e-9
    pl = d['policy_in_loop']
    assert set(pl) == {'reduce32', 'reduce', 'conv'}
    for b in pl.values():
        assert b['consumer_ms'] > 0 and b['ms_per_step'] > b['consumer_ms'] and 0 < b['sweep']['frac'] < 1 and b['guard_moves'] >= 0
        assert abs(b['env_ms_per_step'] - (b['ms_per_step'] - b['consumer_ms'])) < 1e-9 and 'tuner_after' in b
    # round 6: the region timed on the device (value) beside the wall clock around the bracket (value_wall); the CPU baseline measured ALONE on the whole CPU
    # share, the soak beside a second run of it
    assert d['value_wall'] > 0 and d['ms_per_step_wall'] >= d['ms_per_step'] * 0.999 and 'timing' in d and d['per_rank'][0]['barrier_ms'] >= 0 and 'short_episodes_1gpu' in d
    assert len(d['repeats']['value_wall']) == 3 and d['metric_window']['value_wall'] > 0 and wd['value_wall'] > 0
    bs = c['beside_gpu_soak']
    assert bs['cores'] == max(1, c['cores'] - 1) and bs['value'] > 0 and 'nothing else running' in c['sample'] and 'minus 1' in bs['sample']
    sk = d['soak_beside_cpu_baseline']
    assert sk['steps'] >= 256 and sk['value'] > 0 and sk['guard_moves'] >= 0 and c['cores'] >= 1 and c['single_env_one_core']['value'] > 0
    assert len(d['per_rank']) == 1 and d['per_rank'][0]['numa'] == {'skipped': 'single rank'} and d['per_rank_roofline_frac'] == [r['frac']]


@pytest.mark.gpu
def test_bench_plain_run_is_lean_and_dumps_the_last_timed_step(tmp_path):
    """A plain `python bench.py` (no --full) prints the headline alone: the contract's keys and none of --full's blocks.  --dump-outputs writes
    what the last timed step returned as float32 / float64 .npy files within 64 MB, and two runs with the same arguments write identical arrays.
    --steps is the number of timed steps: in the state-only mode with no pre-warm-up and no episode able to time out, the longest-running env
    has taken exactly W + K steps when the arrays are written."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT')}

    def bench(out, *extra):
        p = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--steps', '30', '--warmup', '4', '--dump-outputs', str(tmp_path / out)]
                           + list(extra), env=env, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        lines = [l for l in p.stdout.strip().splitlines() if l.startswith('{')]
        assert len(lines) == 1 and p.stdout.strip().splitlines()[-1] == lines[0], p.stdout
        files = sorted(os.listdir(tmp_path / out))
        return json.loads(lines[0]), {f[:-4]: np.load(tmp_path / out / f) for f in files if f.endswith('.npy')}

    pix = ('--envs-per-gpu', '8192', '--max-steps', '20')
    d, a = bench('a', *pix)
    _, b = bench('b', *pix)
    for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step', 'n_gpus', 'steps', 'warmup', 'config', 'warmup_total'):
        assert k in d, k
    assert d['steps'] == 30 and d['warmup'] == 4 and d['unit'] == 'env-steps/s' and d['dtype'] == 'u8' and d['higher_is_better'] is True
    assert abs(d['value'] - 8192 * 30 / (d['ms_per_step'] * 30e-3)) < 1e-6 * d['value']
    for k in ('roofline', 'kernels_ms', 'repeats', 'metric_window', 'metric_window_desync', 'policy_in_loop', 'cpu_baseline', 'per_rank',
              'other_obs_modes_1gpu', 'short_episodes_1gpu', 'single_env'):
        assert k not in d, k
    assert sorted(a) == sorted(b) == sorted(d['dump_outputs']['arrays'])
    assert {'reward', 'done', 'obs_observation', 'obs_desired_goal', 'obs_init_observation', 'frame_env_index'} <= set(a)
    assert sum(x.nbytes for x in a.values()) == d['dump_outputs']['bytes'] <= 64 << 20
    assert a['reward'].shape == (8192,) and a['obs_observation'].shape == (128, 84, 84, 3) and a['frame_env_index'].shape == (128,)
    for k in a:
        assert a[k].dtype in (np.float32, np.float64) and np.array_equal(a[k], b[k]), k
    assert a['obs_observation'].max() > 0 and a['obs_desired_goal'].max() > 0

    d, s = bench('c', '--obs-mode', 'state', '--envs-per-gpu', '4096', '--max-steps', '1000', '--prewarm-steps', '0')
    assert d['steps'] == 30 and d['warmup_total'] == 4 and s['obs_hdr'].shape == (4096, 16)
    step_num = s['obs_hdr'][:, 8].astype(np.int64) + 256 * s['obs_hdr'][:, 9].astype(np.int64)      # (bytes 8-9: step_num, LE u16)
    assert step_num.max() == 4 + 30, np.bincount(step_num.astype(np.int64))


@pytest.mark.gpu
@pytest.mark.parametrize('name,args,floor_frac,floor_value', [
    ('headline', [], 0.81, 2.80e8),                                     # measured 0.876-0.884 / 3.04-3.07e8 (profiles/r04_clock.txt K)
    ('phases spread out', ['--desync'], 0.80, 2.72e8),                  # 0.859-0.864 / 2.97e8 (round 3: 0.74 / 2.65e8)
    ('32x32', ['--size', '32'], 0.82, 1.27e8),                          # 0.888-0.893 / 1.37e8
    ('AltObs 21x21', ['--raster', 'alt'], 0.79, 4.4e8),                 # 0.849-0.873 / 4.8e8
])
def test_perf_floors_of_the_sweep(name, args, floor_frac, floor_value):
    """The performance of the dominant kernel is a tested property: a fresh `bench.py --full --quick --steps 300` of BASELINE configs[2] (65 536 envs,
    21x21, full frames) -- with the episode phases in step and spread out (~220 envs finish on every step: the steady state of any policy that
    finishes episodes) --, of configs[4]'s 32x32 grids and of the AltObs raster must paint at the given fraction of the 8 TB/s HBM peak at its
    median launch, and step at the given rate: each floor 7-8 % under the committed measurement (profiles/r04_*)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT') and not k.startswith('CW_TUNE_')}
    p = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--full', '--quick', '--steps', '300'] + args, env=env, capture_output=True, text=True,
                       timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    d = json.loads(p.stdout.strip().splitlines()[-1])                # the JSON line is the LAST line of rank 0's stdout
    r = d['roofline']
    assert r['kernel'] == 'cw_render_pieces_kernel' and d['config']['envs_per_gpu'] == 65536
    assert r['frac_at_median_launch'] >= floor_frac, (name, r)
    assert d['value'] >= floor_value, (name, d['value'])


@pytest.mark.gpu
def test_soak_the_clock_and_its_guard_outside_the_bench_loop(monkeypatch):
    """The sweep's clock (7.7 TB/s and its two heads), the busy threshold and the guard were found in bench.py's back-to-back loop on three boxes of one pool
    (DESIGN 4.3).  Here they run where they were NOT tuned: 5 000 steps of the headline batch with the episode phases spread out (~220 envs finish on every
    step), a second engine on the same card taking a step of its own every 50th step, the host never waiting.  The guard may give way (twice at most) but
    must not run away, where it did not move the clock is cw_create's, and over the last 1 000 steps the sweep must still write at >= 0.80 of the HBM peak
    (measured 0.865-0.871: the floor sits 7-8 % under, like test_perf_floors_of_the_sweep's)."""
    from gym_craftingworld_amd import CraftingWorldVecEnv
    for k in list(os.environ):
        if k.startswith('CW_TUNE_'):
            monkeypatch.delenv(k)
    N, T = 65536, 5000
    env = CraftingWorldVecEnv(N, obs_mode='pixels', size=(21, 21), max_steps=300, seed=2024)
    other = CraftingWorldVecEnv(16384, obs_mode='pixels', size=(21, 21), max_steps=300, seed=7)
    env.reset(); other.reset()
    env.set_state(step_num=((np.arange(N) * 7) % 300).astype(np.int32))
    gen = torch.Generator(device='cuda').manual_seed(5)
    acts = torch.randint(0, 6, (256, N), device='cuda', dtype=torch.uint8, generator=gen)
    t0 = env.tuner_state()
    assert t0['period16'] > 0 and t0['guard_slowdowns'] == 0 and t0['period16_head'] > t0['period16'] and t0['period16_busy'] > t0['period16_head']
    for t in range(T - 1000):
        env.step_async(acts[t % 256])
        if t % 50 == 49:
            other.step_async(acts[t % 256][:16384])
    torch.cuda.synchronize()
    t1 = env.tuner_state()
    env.profile_begin(1000)
    for t in range(T - 1000, T):
        env.step_async(acts[t % 256])
        if t % 50 == 49:
            other.step_async(acts[t % 256][:16384])
    torch.cuda.synchronize()
    p = env.profile_end()
    frac = N * (441 + 21168) / (p['ms_render_kernel'] * 1e-3) / 8e12
    print('soak: cw_create %s, after 4000 steps %s; last 1000 sweeps %.4f ms (median %.4f) = %.3f of the peak'
          % (t0, t1, p['ms_render_kernel'], p['ms_render_kernel_median'], frac))
    assert 0 <= t1['guard_slowdowns'] <= 4, (t0, t1)        # (down a notch, back after 64 samples on time, down again: every move counts)
    if t1['guard_slowdowns'] == 0:
        assert 0.93 * t0['period16'] <= t1['period16'] <= t0['period16']      # (cw_create's clock, or a faster one a probe found to pay)
    else:                                                   # (a notch is 0.2 TB/s, ~15 ns of a ~550-ns period: three notches under cw_create's choice at most)
        assert 0.97 * t0['period16'] <= t1['period16'] <= t0['period16'] * 1.09, (t0, t1)
    assert frac >= 0.80, (frac, p, t0, t1)
    assert int(env.counters[1]) > 4 * N                     # (every env finished ~16 episodes on the way: the steady state, not a quiet run)
    env.close(); other.close()


@pytest.mark.gpu
def test_synchronous_calls_do_not_wait_for_another_engines_work():
    """Two engines on one device (MultiDeviceVecEnv, a learner beside an env): a synchronous call on one must not wait for what the OTHER has queued
    (round 4: hipDeviceSynchronize in cw_seed_* / cw_get_mt / cw_get_state / checkpoints stalled everybody).  ~0.6 s of sweeps are queued on B's stream;
    A.get_state() / get_rng_states() / seed() return long before they have run -- and a stream the caller destroyed after use makes the engine fall back to
    one device-wide wait instead of failing."""
    import ctypes as C
    import time
    from gym_craftingworld_amd import CraftingWorldVecEnv
    a = CraftingWorldVecEnv(2048, obs_mode='pixels', size=(9, 9), max_steps=20, seed=1)
    b = CraftingWorldVecEnv(65536, obs_mode='pixels', size=(21, 21), max_steps=300, seed=2)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    acts = torch.randint(0, 6, (65536,), device='cuda', dtype=torch.uint8)
    with torch.cuda.stream(sa):
        a.reset()
        for _ in range(10):
            a.step_async(acts[:2048])
    with torch.cuda.stream(sb):
        b.reset()
    torch.cuda.synchronize()
    with torch.cuda.stream(sb):
        t0 = time.perf_counter()
        for _ in range(3000):                             # ~0.65 s of card time, enqueued in ~50 ms
            b.step_async(acts)
        t_enq = time.perf_counter() - t0
    with torch.cuda.stream(sa):
        t0 = time.perf_counter()
        st = a.get_state()
        t1 = time.perf_counter()
        a.get_rng_states()
        t2 = time.perf_counter()
        a.seed(5)
        t_calls = time.perf_counter() - t0
    torch.cuda.synchronize()
    t_all = time.perf_counter() - t0
    print('enqueue %.3f s; get_state %.3f, get_rng_states %.3f, seed %.3f; everything done after %.3f s' % (t_enq, t1 - t0, t2 - t1, t_calls - (t2 - t0), t_all))
    assert st['grid'].shape == (2048, 9, 9)
    assert t_all > 0.1, (t_enq, t_calls, t_all)           # B still had a lot to do when A's calls began (the enqueue loop runs ahead of the card) ...
    assert t_calls < 0.5 * t_all, (t_enq, t_calls, t_all)  # ... and A's synchronous calls did not sit it out
    # a stream handed to the engine and destroyed by the caller before the next synchronous call: the engine notices and waits for the device instead
    hip = C.CDLL(os.path.join(os.path.dirname(torch.__file__), 'lib', 'libamdhip64.so'))
    s = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(s)) == 0
    assert a._lib.cw_reset(a._h, s) == 0
    for _ in range(5):
        assert a._lib.cw_step(a._h, C.c_void_p(acts.data_ptr()), 2, s) == 0
    assert hip.hipStreamSynchronize(s) == 0 and hip.hipStreamDestroy(s) == 0
    a._settle = lambda: None
    st2 = a.get_state()                                   # (quiesce: hipStreamSynchronize on the dead handle fails -> hipDeviceSynchronize)
    assert int(st2['step_num'].max()) == 5
    a.close(); b.close()
