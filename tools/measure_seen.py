#!/usr/bin/env python3
"""Time cw_seen_insert and VecEnv.reach on one GPU beside the routes that exist without them -> the tables of profiles/r12_seen.txt (stdout).

    python tools/measure_seen.py > profiles/r12_seen.txt

One process, one build.  State-only engines, 21x21, max_steps 300, auto_reset=False.
(a) seen_insert: HIP events around single calls on the caller's stream (a call's launch gap is in the figure), medians (p10 .. p90) of 20 calls after a
    warm-up call.  The rows are the 6 N successors expand() gives N envs ten random steps into their episodes, group = env.  "first call": into a set
    cleared just before (the clear is outside the events); "repeated call": the same rows again, every key held; "16-bit tags": a first call into a set whose
    tags are truncated, with the collisions it counts.  "torch.unique": torch.unique(dim=0, return_inverse=True) over the same keys as int32 [6 N, 9], built
    outside the events -- the route that exists today.  It dedups one batch and has NO MEMORY of earlier calls: it cannot answer the repeated call at all.
(b) reach(): wall time of whole calls (each level synchronises once), envs as reset() leaves them, best of 3.  Depths 6, 12 and 24, then 64 with the
    default max_rows = 2**22, which stops the search where the next frontier would not fit: "searched" is the depth it reached.  Beside it plan() at depth 6,
    the deepest exhaustive search cw_plan allows 65 536 states (events, median of 5).  The frontier sizes per level are reach()'s own."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from gym_craftingworld_amd import CraftingWorldVecEnv  # noqa: E402


def timed(fn, before=None, n=20):
    """one warm-up call, then n timed ones -> (p50, p10, p90) in us; `before` runs ahead of every call, outside the events"""
    def once():
        if before:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3
    once()
    return np.percentile([once() for _ in range(n)], [50, 10, 90])


def cell(p):
    return '%10.1f (%9.1f..%9.1f)' % tuple(p)


def keys_of(hdr, pos, group):
    """the nine key dwords of include/craftingworld.h as int32 [M, 9], in torch"""
    h = hdr.view(torch.int32).reshape(-1, 4)
    p = pos.contiguous().view(torch.int32).reshape(-1, 4)
    return torch.stack([group.to(torch.int32), h[:, 0] & 0x00FFFFFF, h[:, 1], (h[:, 2] >> 17) & 1, h[:, 3], p[:, 0], p[:, 1], p[:, 2], p[:, 3]], dim=1).contiguous()


def insert_table():
    print('# (a) seen_insert: us per call, HIP events around single calls (launch gap included), medians (p10 .. p90) of 20 after a warm-up call')
    print('%-7s %-8s %-16s %34s %10s %10s %10s' % ('N', 'rows', 'call', 'us per call', 'fresh', 'collisions', 'ns/row'))
    for N in (4096, 65536):
        env = CraftingWorldVecEnv(N, size=(21, 21), max_steps=300, obs_mode='state', auto_reset=False, seed=3)
        env.reset()
        warm = torch.randint(0, 6, (10, N), device='cuda', dtype=torch.uint8)
        for t in range(10):
            env.step(warm[t])
        succ = env.expand(fields=('hdr', 'slot_pos'))
        hdr, pos = succ['hdr'].reshape(-1, 16), succ['slot_pos'].reshape(-1, 8)
        M = 6 * N
        group = torch.arange(M, device='cuda', dtype=torch.int32) % N
        keys = keys_of(hdr, pos, group)
        uniq, inverse = torch.unique(keys, dim=0, return_inverse=True)
        for name, bits in (('first call', 0), ('repeated call', 0), ('16-bit tags', 16)):
            env.seen_reserve(2 * M, tag_bits=bits)
            out = env.seen_insert(hdr, pos, group)
            fresh, coll = int(out['fresh'].sum()), env.seen_collisions
            if bits == 0:
                assert fresh == len(uniq) == env.seen_size and coll == 0            # (the two routes count the same keys)
            p = timed(lambda: env.seen_insert(hdr, pos, group, out=out), before=None if name == 'repeated call' else env.seen_clear)
            print('%-7d %-8d %-16s %34s %10d %10d %10.2f' % (N, M, name, cell(p), fresh, coll, p[0] * 1e3 / M))
            sys.stdout.flush()
        p = timed(lambda: torch.unique(keys, dim=0, return_inverse=True))
        print('%-7d %-8d %-16s %34s %10d %10s %10.2f' % (N, M, 'torch.unique', cell(p), len(uniq), '-', p[0] * 1e3 / M))
        env.seen_reserve(0)
        env.close()
        del succ, keys, uniq, inverse
        torch.cuda.empty_cache()


def reach_table():
    print('# (b) reach(): ms per whole call (wall clock, one synchronisation per level), best of 3; plan(6): HIP events, median of 5')
    print('%-7s %-10s %10s %9s %9s %12s   %s' % ('N', 'call', 'ms', 'searched', 'solved', 'states', 'frontier per level'))
    for N in (64, 4096):
        env = CraftingWorldVecEnv(N, size=(21, 21), max_steps=300, obs_mode='state', auto_reset=False, seed=3)
        env.reset()
        env.seen_reserve(1 << 25)
        p = timed(lambda: env.plan(6, fields=('best_q', 'best_action')), n=5)
        solved = int((env.plan(6, fields=('best_q',))['best_q'] > 0).sum())
        print('%-7d %-10s %10.2f %9d %9d %12s   %s' % (N, 'plan(6)', p[0] / 1e3, 6, solved, '-', '-'))
        for D in (6, 12, 24, 64):
            best, r = None, None
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = env.reach(D)
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) * 1e3
                best = dt if best is None else min(best, dt)
            print('%-7d %-10s %10.2f %9d %9d %12d   %s' % (N, 'reach(%d)' % D, best, r['searched_depth'], int((r['distance'] > 0).sum()), r['states'],
                                                           ' '.join(str(f) for f in r['frontier'])))
            if env.seen_overflow or env.seen_collisions:
                print('# (overflow %d, collisions %d: states expanded again, results exact)' % (env.seen_overflow, env.seen_collisions))
            sys.stdout.flush()
        env.close()
        torch.cuda.empty_cache()


def main():
    print('# cw_seen_insert (VecEnv.seen_insert) and VecEnv.reach on one %s; obs_mode=state, 21x21, max_steps 300, auto_reset=False' % torch.cuda.get_device_name(0))
    insert_table()
    reach_table()


if __name__ == '__main__':
    main()
