#!/usr/bin/env python3
"""Time cw_snapshot_save / cw_snapshot_load on one GPU beside the host path they replace -> the table of profiles/snapshot.txt (stdout).

    python tools/measure_snapshot.py > profiles/snapshot.txt

HIP events around single calls on the caller's stream (a call's launch gap is in the figure), medians (p10 .. p90) after a warm-up of every shape, one
process.  65 536 envs, 21x21, auto-reset (look-ahead records kept: a row holds the ring too).  get_state() + set_state() -- the only way to put an env back
before the bank existed, unchanged by it -- is synchronous and moves the whole batch: a host clock around the pair."""
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
    print('# cw_snapshot_save / cw_snapshot_load (VecEnv.snapshot_save / snapshot_load) on one %s: us per call, HIP events around single calls on the'
          % torch.cuda.get_device_name(0))
    print("# caller's stream (launch gap included), medians (p10 .. p90) of 200 calls (65 536 selected: 40) after a warm-up of every shape, one process.")
    print('# %d envs, 21x21, max_steps 300, auto_reset=True (look-ahead records kept), a bank of %d rows; the row array is a device tensor handed over in place.' % (N, N))
    print('# "load": with the stream (an exact twin); "load episode": with_stream=False; "fork": every selected env loads the SAME row.')
    print('%-8s %-14s %28s %28s' % ('obs_mode', 'call', '219 selected', '65536 selected'))
    rng = np.random.RandomState(1)
    sparse = np.full(N, -1, np.int32)
    pick = rng.choice(N, 219, replace=False)
    sparse[pick] = pick
    for obs_mode in ('state', 'pixels'):
        env = CraftingWorldVecEnv(N, size=(21, 21), max_steps=300, obs_mode=obs_mode, seed=3)
        env.snapshot_reserve(N)
        env.reset()
        acts = torch.randint(0, 4, (10, N), device='cuda', dtype=torch.uint8)
        for t in range(10):
            env.step(acts[t])
        rows = {219: torch.as_tensor(sparse, device='cuda'), N: torch.arange(N, dtype=torch.int32, device='cuda')}
        fork = {k: torch.where(v >= 0, torch.full_like(v, int(pick[0])), v) for k, v in rows.items()}
        env.snapshot_save(rows[N])                                # (every row valid before the first load is timed)
        calls = [('save', lambda k: env.snapshot_save(rows[k])),
                 ('load', lambda k: env.snapshot_load(rows[k])),
                 ('load episode', lambda k: env.snapshot_load(rows[k], with_stream=False)),
                 ('fork', lambda k: env.snapshot_load(fork[k]))]
        for name, fn in calls:
            row = [timed(lambda: fn(k), 200 if k == 219 else 40) for k in (219, N)]
            print('%-8s %-14s %28s %28s' % (obs_mode, name, cell(row[0]), cell(row[1])))
        print('# row: %d bytes' % env.snapshot_row_bytes)
        ts = []
        for i in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st = env.get_state()
            env.set_state(**st)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        ts = ts[1:]
        print('%-8s get_state() + set_state(), all %d envs (the streams not among them): %8.2f ms (%8.2f..%8.2f), host clock, median (min .. max) of 3'
              % (obs_mode, N, np.median(ts), min(ts), max(ts)))
        env.close()
        del env


if __name__ == '__main__':
    main()
