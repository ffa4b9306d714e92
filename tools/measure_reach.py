#!/usr/bin/env python3
"""Time VecEnv.reach_async (cw_reach) beside VecEnv.reach on one GPU -> the table of profiles/r13_reach.txt (stdout).

    python tools/measure_reach.py [--parent DIR] > profiles/r13_reach.txt

State-only engines, 21x21, max_steps 300, auto_reset=False, envs as reset() leaves them: the shapes of profiles/r12_seen.txt (b) -- 64 envs at depths
6 / 12 / 24 and 4 096 envs at depths 6 / 12 / 16 -- with a visited set for 2**25 keys.
  reach()        wall time of whole calls (one synchronisation per level), best of 3, on this build; with --parent DIR (a checkout of the parent commit
                 with its library built) also on that build, measured by this file run from DIR in a child process.
  reach_async    HIP events around single calls on the caller's stream (the launch gaps are in the figure), median (p10 .. p90) of 10 after a warm-up
                 call; "graph": the same call captured into a graph, events around single replays.  Twice: with the default workspace (max_rows =
                 2**22, whose launch shapes every level pays whatever its frontier holds) and with one FITTED to the search (max_rows = the next power of
                 two above its largest frontier).
  no-op level    a call whose start rows all take no part (env_of = -1), divided by max_depth: what a level over an empty frontier costs -- its launches.
Every reach_async result is compared with reach()'s before it is timed."""
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.environ.get('CW_MEASURE_ROOT') or os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
from gym_craftingworld_amd import CraftingWorldVecEnv  # noqa: E402

SHAPES = ((64, (6, 12, 24)), (4096, (6, 12, 16)))
SET = 1 << 25


def timed(fn, n=10):
    """one warm-up call, then n timed ones -> (p50, p10, p90) in ms"""
    def once():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)
    once()
    return np.percentile([once() for _ in range(n)], [50, 10, 90])


def cell(p):
    return '%8.3f (%8.3f..%8.3f)' % tuple(p)


def wall(env, D):
    best, r = None, None
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = env.reach(D)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
    return best, r


def make(N):
    env = CraftingWorldVecEnv(N, size=(21, 21), max_steps=300, obs_mode='state', auto_reset=False, seed=3)
    env.reset()
    env.seen_reserve(SET)
    return env


def reach_only():
    """the child's part: reach() alone, on whatever build ROOT holds"""
    for N, depths in SHAPES:
        env = make(N)
        for D in depths:
            print('REACH %d %d %.3f' % (N, D, wall(env, D)[0]))
            sys.stdout.flush()
        env.close()
        torch.cuda.empty_cache()


def parent_times(tree):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), '--reach-only'], env=dict(os.environ, CW_MEASURE_ROOT=os.path.abspath(tree)),
                         capture_output=True, text=True, timeout=900, check=True).stdout
    return {(int(f[1]), int(f[2])): float(f[3]) for f in (l.split() for l in out.splitlines()) if f and f[0] == 'REACH'}


def main():
    parent = parent_times(sys.argv[sys.argv.index('--parent') + 1]) if '--parent' in sys.argv else {}
    print('# VecEnv.reach_async (cw_reach) beside VecEnv.reach on one %s; obs_mode=state, 21x21, max_steps 300, auto_reset=False, a set for 2**25 keys' %
          torch.cuda.get_device_name(0))
    print('# ms per whole call.  reach(): wall clock, best of 3 (parent: the parent commit\'s build).  reach_async and its graph replay: HIP events around single')
    print('# calls, median (p10 .. p90) of 10.  no-op level: a call whose start rows all take no part, divided by max_depth, in us.')
    print('%-6s %-6s %-9s %9s %9s %30s %30s %11s %9s %7s %10s' % ('N', 'depth', 'max_rows', 'reach()', 'parent', 'reach_async', 'graph replay', 'no-op us/lvl',
                                                                   'searched', 'solved', 'states'))
    for N, depths in SHAPES:
        env = make(N)
        none = torch.full((N,), -1, dtype=torch.int32, device='cuda')
        for D in depths:
            ms, ref = wall(env, D)
            fitted = 1 << int(np.ceil(np.log2(max(max(ref['frontier']), N) + 1)))
            for max_rows in (1 << 22, fitted):
                env.reach_reserve(max_rows, D)
                out = env.reach_async(D)
                torch.cuda.synchronize()
                assert torch.equal(out['distance'], ref['distance']) and torch.equal(out['plan'], ref['plan']) and int(out['states'][0]) == ref['states']
                assert out['frontier'].cpu().numpy().tolist()[:len(ref['frontier'])] == ref['frontier'] and int(out['searched_depth'][0]) == ref['searched_depth']
                assert (env.seen_overflow, env.seen_collisions) == (0, 0)
                p = timed(lambda: env.reach_async(D, out=out))
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    env.reach_async(D, out=out)
                q = timed(g.replay)
                idle = env.reach_async(D, env.hdr, env.slot_pos, none)
                z = timed(lambda: env.reach_async(D, env.hdr, env.slot_pos, none, out=idle))
                print('%-6d %-6d %-9d %9.3f %9s %30s %30s %11.1f %9d %7d %10d' % (
                    N, D, max_rows, ms, '%9.3f' % parent[(N, D)] if (N, D) in parent else '-', cell(p), cell(q), z[0] * 1e3 / D, ref['searched_depth'],
                    int((ref['distance'] > 0).sum()), ref['states']))
                print('#   frontier per level: %s; workspace %.1f MB' % (' '.join(str(f) for f in ref['frontier']), env.reach_bytes / 1e6))
                sys.stdout.flush()
                del g
        env.reach_reserve(0, 1)
        env.close()
        torch.cuda.empty_cache()


if __name__ == '__main__':
    reach_only() if '--reach-only' in sys.argv else main()
