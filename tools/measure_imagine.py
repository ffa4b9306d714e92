#!/usr/bin/env python3
"""Time cw_imagine_masked beside cw_reset_masked on one GPU -> the table of profiles/r08_imagine.txt (stdout).

    python tools/measure_imagine.py > profiles/r08_imagine.txt

HIP events around single calls on the caller's stream (a call's launch gap is in the figure), medians (p10 .. p90) after a warm-up of every shape, one
process.  65 536 envs, 21x21.  The rewind path of an engine that keeps look-ahead records is synchronous: a host clock around the call."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from gym_craftingworld_amd import CraftingWorldVecEnv  # noqa: E402


def timed(fn, n, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return np.percentile(out, [50, 10, 90])


def cell(p):
    return '%8.1f (%7.1f..%7.1f)' % tuple(p)


def main():
    N = 65536
    print('# cw_imagine_masked / VecEnv.imagine_obs beside cw_reset_masked / VecEnv.reset_envs on one %s: us per call, HIP events around single calls on the'
          % torch.cuda.get_device_name(0))
    print("# caller's stream (launch gap included), medians (p10 .. p90) of 200 calls (65 536 selected: 40) after a warm-up of every shape, one process.")
    print('# %d envs, 21x21, max_steps 300, auto_reset=False (no look-ahead records: one kernel per call).  imagine: each env\'s own desired mask;' % N)
    print('# "commit": the goal records stored and, in pixels, the desired_goal frame repainted; "frames": the goal frames written to a caller\'s array.')
    print('%-8s %-22s %28s %28s' % ('obs_mode', 'call', '219 selected', '65536 selected'))
    rng = np.random.RandomState(1)
    sparse = np.zeros(N, bool)
    sparse[rng.choice(N, 219, replace=False)] = True
    for obs_mode in ('state', 'pixels'):
        env = CraftingWorldVecEnv(N, size=(21, 21), max_steps=300, obs_mode=obs_mode, seed=3, auto_reset=False)
        env.reset()
        acts = torch.randint(0, 4, (10, N), device='cuda', dtype=torch.uint8)
        for t in range(10):
            env.step(acts[t])
        masks = {219: torch.as_tensor(sparse, device='cuda'), N: torch.ones(N, dtype=torch.bool, device='cuda')}
        out = torch.zeros((N,) + env.frame_shape, dtype=torch.uint8, device='cuda')
        calls = [('imagine commit', lambda m: env._lib.cw_imagine_masked(env._h, m.data_ptr(), None, 1, None, None, env._stream())),
                 ('imagine frames', lambda m: env.imagine_obs(m, out=out)),
                 ('imagine commit+frames', lambda m: env.imagine_obs(m, commit=True, out=out)),
                 ('reset_envs', lambda m: env.reset_envs(m))]
        for name, fn in calls:
            row = [timed(lambda: fn(masks[k]), 200 if k == 219 else 40) for k in (219, N)]
            print('%-8s %-22s %28s %28s' % (obs_mode, name, cell(row[0]), cell(row[1])))
        env.close()
        del env, out
    print('# The rewind path: imagine_obs(219 selected, commit) on an auto_reset=True engine (look-ahead records kept): cw_get_mt + cw_seed_mt + the kernel,')
    print('# synchronous; host clock around the call and a device synchronise, ms per call, median (min .. max) of 5 after one warm-up; state mode.')
    for n in (4096, N):
        env = CraftingWorldVecEnv(n, size=(21, 21), max_steps=300, obs_mode='state', seed=3, auto_reset=True)
        env.reset()
        m = torch.zeros(n, dtype=torch.bool, device='cuda')
        m[torch.as_tensor(rng.choice(n, 219, replace=False), device='cuda')] = True
        ts = []
        for i in range(6):
            env.step(torch.zeros(n, dtype=torch.uint8, device='cuda'))      # (records are parked again: the refill after a rewind covers the whole batch)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            env.imagine_obs(m, commit=True)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        ts = ts[1:]
        print('rewind   %6d envs   %8.2f ms (%8.2f..%8.2f)' % (n, np.median(ts), min(ts), max(ts)))
        env.close()


if __name__ == '__main__':
    main()
