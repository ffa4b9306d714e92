#!/usr/bin/env python3
"""Time cw_expand on one GPU beside the calls it replaces -> the table of profiles/r07_expand.txt (stdout).

    python tools/measure_expand.py > profiles/r07_expand.txt

HIP events around single calls on the caller's stream (a call's launch gap is in the figure), medians (p10 .. p90) of 200 calls after a warm-up, one
process, one build.  A state-only engine, 21x21, auto_reset=False, at 4 096 and 65 536 envs.  "the long way": the same six successors through the calls
that existed before -- one snapshot_save, then six times snapshot_load(with_stream=True) + step + clones of hdr, slot_pos, reward and done."""
import os
import sys

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
    sizes = (4096, 65536)
    print('# cw_expand (VecEnv.expand) on one %s: us per call, HIP events around single calls on the caller\'s stream (launch gap included),'
          % torch.cuda.get_device_name(0))
    print('# medians (p10 .. p90) of 200 calls after a warm-up of every shape, one process.  obs_mode=state, 21x21, max_steps 300, auto_reset=False.')
    print('# "expand": all six fields into buffers of the caller\'s (out=...); "expand, outputs only": reward, done, changed, achieved_mask;')
    print('# "depth 2": the 6 N successor records fed back, 36 N rows; "the long way": snapshot_save + 6 x (snapshot_load + step + 4 clones).')
    print('%-24s %28s %28s' % ('call', '%d envs' % sizes[0], '%d envs' % sizes[1]))
    rows = {}
    for N in sizes:
        env = CraftingWorldVecEnv(N, size=(21, 21), max_steps=300, obs_mode='state', auto_reset=False, seed=3)
        env.snapshot_reserve(N)
        env.reset()
        acts = torch.randint(0, 6, (10, N), device='cuda', dtype=torch.uint8)
        for t in range(10):
            env.step(acts[t])
        out = env.expand()
        few = ('reward', 'done', 'changed', 'achieved_mask')
        out_few = {k: out[k] for k in few}
        out2 = env.expand(hdr=out['hdr'], slot_pos=out['slot_pos'])
        ids = torch.arange(N, dtype=torch.int32, device='cuda')
        six = [torch.full((N,), a, dtype=torch.uint8, device='cuda') for a in range(6)]

        def long_way():
            env.snapshot_save(ids)
            kept = []
            for a in range(6):
                env.snapshot_load(ids, with_stream=True)
                env.step(six[a])
                kept.append((env.hdr.clone(), env.slot_pos.clone(), env.reward.clone(), env.done.clone()))
            env.snapshot_load(ids, with_stream=True)              # (the envs back where they were: what expand never moved)
            return kept

        calls = [('expand', lambda: env.expand(out=out)),
                 ('expand, outputs only', lambda: env.expand(fields=few, out=out_few)),
                 ('depth 2', lambda: env.expand(hdr=out['hdr'], slot_pos=out['slot_pos'], out=out2)),
                 ('the long way', long_way)]
        for name, fn in calls:
            rows.setdefault(name, []).append(timed(fn, 200))
        env.close()
        del env
    for name, r in rows.items():
        print('%-24s %28s %28s' % (name, cell(r[0]), cell(r[1])))


if __name__ == '__main__':
    main()
