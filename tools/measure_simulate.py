#!/usr/bin/env python3
"""Time cw_simulate on one GPU beside the route it replaces -> the table of profiles/r08_simulate.txt (stdout).

    python tools/measure_simulate.py > profiles/r08_simulate.txt

HIP events around single calls on the caller's stream (a call's launch gap is in the figure), medians (p10 .. p90) after a warm-up of every shape, one
process, one build.  A state-only engine, 21x21, max_steps 300, auto_reset=False, 65 536 envs; K plans per env (the broadcast form, M = K x 65 536
states), T steps.  "by expand": the same final records, returns and traces by the route that existed before -- T rounds of expand(hdr=, slot_pos=,
fields=('reward', 'done', 'hdr', 'slot_pos')), six successors each, plus the gather of the chosen action's rows.  Last, for orientation, the state-only
rollout() of an auto-reset engine of the same size per env-step."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from gym_craftingworld_amd import CraftingWorldVecEnv  # noqa: E402
from gym_craftingworld_amd.vec_env import SIMULATE_FIELDS  # noqa: E402

N = 65536


def timed(fn, n, warm=3):
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
    return '%9.1f (%8.1f..%8.1f)' % tuple(p)


def main():
    print('# cw_simulate (VecEnv.simulate) on one %s: us per call, HIP events around single calls on the caller\'s stream (launch gap included),'
          % torch.cuda.get_device_name(0))
    print('# medians (p10 .. p90) of 100 calls (by expand: 10) after a warm-up of every shape, one process.  obs_mode=state, 21x21, max_steps 300,')
    print('# auto_reset=False, %d envs, K plans per env broadcast (M = K x N states), T steps, random actions 0..5, out= buffers of the caller\'s.' % N)
    print('# "simulate": the six per-state fields; "+ traces": rewards and dones [T, M] too; "stop" / "on": stop_at_done True / False;')
    print('# "by expand": T x expand(fields=reward, done, hdr, slot_pos) + the gather of the chosen rows (all T steps, as "on"); ns/step: per state-step.')
    print('%-6s %-6s %-22s %32s %10s' % ('K', 'T', 'call', 'us per call', 'ns/step'))
    env = CraftingWorldVecEnv(N, size=(21, 21), max_steps=300, obs_mode='state', auto_reset=False, seed=3)
    env.reset()
    warm = torch.randint(0, 6, (10, N), device='cuda', dtype=torch.uint8)
    for t in range(10):
        env.step(warm[t])
    for K in (1, 16):
        M = K * N
        cols = torch.arange(M, device='cuda')
        h0, p0 = env.hdr.repeat(K, 1), env.slot_pos.repeat(K, 1)
        ex = env.expand(hdr=h0, slot_pos=p0, fields=('reward', 'done', 'hdr', 'slot_pos'))
        for T in (8, 64):
            acts = torch.randint(0, 6, (T, M), device='cuda', dtype=torch.uint8)
            idx = acts.long()
            out6 = env.simulate(acts, fields=SIMULATE_FIELDS[:6])
            out8 = env.simulate(acts, fields=SIMULATE_FIELDS)
            rew, don = torch.empty((T, M), dtype=torch.int32, device='cuda'), torch.empty((T, M), dtype=torch.bool, device='cuda')

            def by_expand():
                h, p = h0, p0
                for t in range(T):
                    env.expand(hdr=h, slot_pos=p, fields=('reward', 'done', 'hdr', 'slot_pos'), out=ex)
                    a = idx[t]
                    h, p, rew[t], don[t] = ex['hdr'][a, cols], ex['slot_pos'][a, cols], ex['reward'][a, cols], ex['done'][a, cols]
                return h, p, rew.sum(dim=0)

            calls = [('simulate, stop', lambda: env.simulate(acts, stop_at_done=True, fields=SIMULATE_FIELDS[:6], out=out6), 100),
                     ('simulate, on', lambda: env.simulate(acts, stop_at_done=False, fields=SIMULATE_FIELDS[:6], out=out6), 100),
                     ('+ traces, stop', lambda: env.simulate(acts, stop_at_done=True, fields=SIMULATE_FIELDS, out=out8), 100),
                     ('+ traces, on', lambda: env.simulate(acts, stop_at_done=False, fields=SIMULATE_FIELDS, out=out8), 100),
                     ('by expand', by_expand, 10)]
            for name, fn, reps in calls:
                p = timed(fn, reps)
                print('%-6d %-6d %-22s %32s %10.3f' % (K, T, name, cell(p), p[0] * 1e3 / (T * M)))
                sys.stdout.flush()
    env.close()
    env = CraftingWorldVecEnv(N, size=(21, 21), max_steps=300, obs_mode='state', seed=3)
    env.reset()
    for T in (8, 64):
        acts = torch.randint(0, 6, (T, N), device='cuda', dtype=torch.uint8)
        p = timed(lambda: env.rollout(acts, record=True), 100)
        print('%-6s %-6d %-22s %32s %10.3f' % ('-', T, 'rollout (auto-reset)', cell(p), p[0] * 1e3 / (T * N)))
    env.close()


if __name__ == '__main__':
    main()
