#!/usr/bin/env python3
"""Time cw_load_records on one GPU beside cw_snapshot_load(with_stream=0) of the same envs in the same run -> the table of profiles/r13_load_records.txt.

    python tools/measure_load_records.py              the table on stdout
    python tools/measure_load_records.py --write      ... and into profiles/r13_load_records.txt

HIP events around single calls on the caller's stream (a call's launch gap is in the figure), medians (p10 .. p90) after a warm-up of every shape, one
process.  65 536 envs, 21x21, auto-reset, the state and the dirty-cell modes.  The records are a clone of the engine's own hdr / slot_pos, the index array a
device tensor handed over in place; "load episode" is the snapshot bank's way to the same state (a row holds the start and goal states too, and the kernel
paints all three frames where load_records paints one)."""
import io
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
from gym_craftingworld_amd import CraftingWorldVecEnv  # noqa: E402

RECORD = os.path.join(ROOT, 'profiles', 'r13_load_records.txt')


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


def main(out):
    N = 65536
    say = lambda line: print(line, file=out)  # noqa: E731
    say('# cw_load_records (VecEnv.load_records) beside cw_snapshot_load(with_stream=0) on one %s: us per call, HIP events around single calls on the'
        % torch.cuda.get_device_name(0))
    say("# caller's stream (launch gap included), medians (p10 .. p90) of 200 calls (65 536 selected: 40) after a warm-up of every shape, one process.")
    say('# %d envs, 21x21, max_steps 300, auto_reset=True; %d records (a clone of hdr / slot_pos), a bank of %d rows; index and row arrays are device' % (N, N, N))
    say('# tensors handed over in place.  "permuted": env i takes record / row perm[i]; "one record": every selected env takes the same one; "+ status": with')
    say('# the status bytes written.')
    say('%-13s %-26s %28s %28s' % ('obs_mode', 'call', '219 selected', '65536 selected'))
    rng = np.random.RandomState(1)
    sparse = np.full(N, -1, np.int32)
    pick = rng.choice(N, 219, replace=False)
    sparse[pick] = pick
    perm = rng.permutation(N).astype(np.int32)
    for obs_mode in ('state', 'pixels_dirty'):
        env = CraftingWorldVecEnv(N, size=(21, 21), max_steps=300, obs_mode=obs_mode, seed=3)
        env.snapshot_reserve(N)
        env.reset()
        acts = torch.randint(0, 6, (10, N), device='cuda', dtype=torch.uint8)
        for t in range(10):
            env.step(acts[t])
        rec_h, rec_p = env.hdr.clone(), env.slot_pos.clone()
        own = {219: torch.as_tensor(sparse, device='cuda'), N: torch.arange(N, dtype=torch.int32, device='cuda')}
        permuted = {219: torch.as_tensor(np.where(sparse >= 0, perm, -1).astype(np.int32), device='cuda'), N: torch.as_tensor(perm, device='cuda')}
        one = {k: torch.where(v >= 0, torch.full_like(v, int(pick[0])), v) for k, v in own.items()}
        env.snapshot_save(own[N])                                 # (every row valid before the first load is timed)
        calls = [('load_records', lambda k: env.load_records(rec_h, rec_p, own[k])),
                 ('load_records permuted', lambda k: env.load_records(rec_h, rec_p, permuted[k])),
                 ('load_records one record', lambda k: env.load_records(rec_h, rec_p, one[k])),
                 ('load_records + status', lambda k: env.load_records(rec_h, rec_p, own[k], status=True)),
                 ('snapshot load episode', lambda k: env.snapshot_load(own[k], with_stream=False)),
                 ('snapshot load ep. permuted', lambda k: env.snapshot_load(permuted[k], with_stream=False))]
        for name, fn in calls:
            row = [timed(lambda: fn(k), 200 if k == 219 else 40) for k in (219, N)]
            say('%-13s %-26s %28s %28s' % (obs_mode, name, cell(row[0]), cell(row[1])))
        say('# a record: 32 bytes; a bank row: %d bytes; envs skipped by all of the above: %d' % (env.snapshot_row_bytes, env.snapshot_skipped))
        env.close()
        del env


if __name__ == '__main__':
    buf = io.StringIO()
    main(buf)
    sys.stdout.write(buf.getvalue())
    if '--write' in sys.argv:
        with open(RECORD, 'w') as f:
            f.write(buf.getvalue())
