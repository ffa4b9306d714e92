#!/usr/bin/env python3
"""Time cw_unroll on one GPU beside the route it replaces and beside its two floors -> the table of profiles/r16_unroll.txt (stdout).

    python tools/measure_unroll.py > profiles/r16_unroll.txt

HIP events around single calls on the caller's stream (a call's launch gap is in the figure), medians (p10 .. p90) after a warm-up of every shape, one
process, one build.  State-only engines, 21x21, max_steps 300 (goals out of reach within T), auto_reset=False, 4 096 and 65 536 envs; K plans per env (the
broadcast form, M = K x N states), T steps.  Five columns per shape:
  (a) unroll       unroll() with all seven fields
  (b) traces       unroll() with reward, done, changed, taken and length only: the step loop without the record stores
  (c) by simulate  the route a caller had before: T one-step simulate() calls fed back into each other, each writing its records, reward and done straight
                   into its slice of preallocated [T + 1, M, ...] / [T, M] tensors (row 0 copied in first)
  (d) simulate     simulate() of the same shape, the six per-state fields: the kernel cannot be faster than its own compute
  (e) fill         one fill_ of as many bytes as (a) writes: it cannot be faster than its own stores"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from gym_craftingworld_amd import CraftingWorldVecEnv  # noqa: E402
from gym_craftingworld_amd.vec_env import SIMULATE_FIELDS, UNROLL_FIELDS  # noqa: E402

TRACES = ('reward', 'done', 'changed', 'taken', 'length')
ONE_STEP = ('hdr', 'slot_pos', 'rewards', 'dones')


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
    print('# cw_unroll (VecEnv.unroll) on one %s: us per call, HIP events around single calls on the caller\'s stream (launch gap included),'
          % torch.cuda.get_device_name(0))
    print('# medians (p10 .. p90) of 50 calls (by simulate: 10) after a warm-up of every shape, one process.  obs_mode=state, 21x21, max_steps 300,')
    print('# auto_reset=False, N envs, K plans per env broadcast (M = K x N states), T steps, random actions 0..5, stop_at_done=True, out= buffers of the')
    print('# caller\'s.  (a) unroll: all seven fields; (b) traces: reward, done, changed, taken, length; (c) by simulate: T one-step simulate() calls, each')
    print('# writing hdr, slot_pos, rewards, dones into its slice of preallocated [T + 1, M] / [T, M] tensors; (d) simulate: the same shape, six per-state')
    print('# fields; (e) fill: one fill_ of the bytes (a) writes.  MB: those bytes; a/c: (a) over (c); a/(d+e): (a) over the sum of its two floors.')
    print('%-6s %-3s %-3s %8s  %-12s %32s' % ('N', 'K', 'T', 'MB', 'call', 'us per call'))
    for N in (4096, 65536):
        env = CraftingWorldVecEnv(N, size=(21, 21), max_steps=300, obs_mode='state', auto_reset=False, seed=3)
        env.reset()
        warm = torch.randint(0, 6, (10, N), device='cuda', dtype=torch.uint8)
        for t in range(10):
            env.step(warm[t])
        for K in (1, 16):
            M = K * N
            h0, p0 = env.hdr.repeat(K, 1), env.slot_pos.repeat(K, 1)
            env_of = (torch.arange(M, device='cuda') % N).to(torch.int32)
            for T in (8, 64):
                acts = torch.randint(0, 6, (T, M), device='cuda', dtype=torch.uint8)
                full = env.unroll(acts)
                small = env.unroll(acts, fields=TRACES)
                out6 = env.simulate(acts, fields=SIMULATE_FIELDS[:6])
                n_bytes = sum(t.numel() * t.element_size() for t in full.values())
                blob = torch.empty(n_bytes, dtype=torch.uint8, device='cuda')
                H, P = torch.empty_like(full['hdr']), torch.empty_like(full['slot_pos'])
                R, D = torch.empty((T, M), dtype=torch.int32, device='cuda'), torch.empty((T, M), dtype=torch.bool, device='cuda')
                steps = [dict(hdr=H[t + 1], slot_pos=P[t + 1], rewards=R[t:t + 1], dones=D[t:t + 1]) for t in range(T)]

                def by_simulate():
                    H[0].copy_(h0)
                    P[0].copy_(p0)
                    for t in range(T):
                        env.simulate(acts[t:t + 1], H[t], P[t], env_of, stop_at_done=False, fields=ONE_STEP, out=steps[t])

                by_simulate()
                torch.cuda.synchronize()
                off = env.unroll(acts, stop_at_done=False)                       # (the route is right: the same records and traces)
                assert torch.equal(H, off['hdr']) and torch.equal(P, off['slot_pos']) and torch.equal(R, off['reward']) and torch.equal(D, off['done'])
                del off
                calls = [('(a) unroll', lambda: env.unroll(acts, fields=UNROLL_FIELDS, out=full), 50),
                         ('(b) traces', lambda: env.unroll(acts, fields=TRACES, out=small), 50),
                         ('(c) by simulate', by_simulate, 10),
                         ('(d) simulate', lambda: env.simulate(acts, fields=SIMULATE_FIELDS[:6], out=out6), 50),
                         ('(e) fill', lambda: blob.fill_(0), 50)]
                med = {}
                for name, fn, reps in calls:
                    p = timed(fn, reps)
                    med[name[1]] = p[0]
                    print('%-6d %-3d %-3d %8.1f  %-16s %32s' % (N, K, T, n_bytes / 1e6, name, cell(p)))
                    sys.stdout.flush()
                print('%-6d %-3d %-3d %8s  a/c %.2f   a/(d+e) %.2f   %.0f GB/s written by (a)' % (N, K, T, '', med['a'] / med['c'], med['a'] / (med['d'] + med['e']),
                                                                                                   n_bytes / med['a'] / 1e3))
                del full, small, out6, blob, H, P, R, D, steps
        env.close()


if __name__ == '__main__':
    main()
