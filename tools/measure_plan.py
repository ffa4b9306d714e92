#!/usr/bin/env python3
"""Time cw_plan on one GPU beside the route it replaces -> the table of profiles/r10_plan.txt (stdout).

    python tools/measure_plan.py > profiles/r10_plan.txt

HIP events around single calls on the caller's stream (a call's launch gap is in the figure), medians (p10 .. p90) after a warm-up call of every shape,
one process, one build.  A state-only engine, 21x21, max_steps 300, auto_reset=False, 4 096 and 65 536 envs ten random steps into their episodes, the
depths in ascending order; the run of a batch size stops at the first call above 2 s.  "far": the goals reset() drew, out of reach within the horizon --
no plan ends, nothing is pruned, the whole tree of 6 + 36 + ... + 6^D steps per state is walked: the worst case.  "near": every env's goal is the achieved
mask three random steps reach, so that most searches find a success early and prune.  "enumerated": the same seven results by the route that existed
before -- simulate() of the envs' own states broadcast over all 6^D strings (the action tensor built once, outside the timing) plus the reduction in
torch (maximum, smallest maximiser, gather of its rows, zeroed plan tail) -- at the depths whose 6^D x N states stay under simulate()'s cap of 2^27."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from gym_craftingworld_amd import CraftingWorldVecEnv  # noqa: E402
from gym_craftingworld_amd.vec_env import PLAN_FIELDS  # noqa: E402

KERNEL_FIELDS = PLAN_FIELDS[:7]
LIMIT_US = 2e6


def timed(fn, limit_us=LIMIT_US):
    """one warm-up call, then 20 timed ones (5 above 10 ms a call, 1 above the limit) -> (p50, p10, p90) in us"""
    def once():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3
    first = once()
    if first > limit_us:
        return np.array([first, first, first])
    out = [once() for _ in range(20 if first < 1e4 else 5)]
    return np.percentile(out, [50, 10, 90])


def cell(p):
    return '%11.1f (%10.1f..%10.1f)' % tuple(p)


def strings(D, N):
    """all 6^D strings for each of N envs as simulate()'s broadcast form takes them: uint8 [D, 6^D, N]"""
    s = torch.arange(6 ** D, device='cuda')
    digits = torch.stack([(s // 6 ** (D - 1 - t)) % 6 for t in range(D)]).to(torch.uint8)
    return digits[:, :, None].expand(D, 6 ** D, N).contiguous()


def enumerated(env, D, acts, sim_out):
    N, n = env.num_envs, 6 ** D
    r = env.simulate(acts, out=sim_out)
    ret = r['ret'].view(6, n // 6, N)
    q = ret.amax(dim=1)
    first = torch.where(ret == q[:, None, :], torch.arange(n // 6, device='cuda')[None, :, None], n).amin(dim=1) + torch.arange(6, device='cuda')[:, None] * (n // 6)
    flat = first * N + torch.arange(N, device='cuda')[None, :]
    out = {f: r[f][flat] for f in ('length', 'done', 'achieved_mask', 'hdr', 'slot_pos')}
    plan = torch.stack([(first // 6 ** (D - 1 - t)) % 6 for t in range(D)], dim=1)
    out['plan'] = torch.where(torch.arange(D, device='cuda')[None, :, None] < out['length'][:, None, :], plan, 0).to(torch.uint8)
    out['q'] = q
    return out


def main():
    print('# cw_plan (VecEnv.plan) on one %s: us per call, HIP events around single calls on the caller\'s stream (launch gap included), medians (p10 .. p90)'
          % torch.cuda.get_device_name(0))
    print('# of 20 calls (5 above 10 ms, 1 above 2 s: the run of that batch size ends there) after a warm-up call, one process.  obs_mode=state, 21x21, max_steps 300,')
    print('# auto_reset=False, N envs ten random steps in, all seven kernel fields into out= buffers.  far: no goal within the horizon, the whole tree is walked;')
    print('# near: goals three random steps away, most searches prune; enumerated: simulate() of all 6^D strings (broadcast) + the torch reduction, goals far.')
    print('# steps/state: 6 + 36 + ... + 6^D, what the far search walks; ns/step: the far figure per state-step.')
    print('%-7s %-3s %-12s %38s %12s %10s' % ('N', 'D', 'call', 'us per call', 'steps/state', 'ns/step'))
    for N in (4096, 65536):
        env = CraftingWorldVecEnv(N, size=(21, 21), max_steps=300, obs_mode='state', auto_reset=False, seed=3)
        env.reset()
        warm = torch.randint(0, 6, (10, N), device='cuda', dtype=torch.uint8)
        for t in range(10):
            env.step(warm[t])
        far = env.get_state()['desired'].astype(np.uint16)
        near = env.simulate(torch.randint(0, 6, (3, N), device='cuda', dtype=torch.uint8), stop_at_done=False)['achieved_mask'].cpu().numpy().view(np.uint16)
        stop = False
        for D in range(1, 7):
            out = env.plan(D, fields=KERNEL_FIELDS)
            steps = sum(6 ** d for d in range(1, D + 1))
            for name, goals in (('plan, far', far), ('plan, near', near)):
                env.set_state(desired=goals)
                p = timed(lambda: env.plan(D, fields=KERNEL_FIELDS, out=out))
                print('%-7d %-3d %-12s %38s %12d %10s' % (N, D, name, cell(p), steps, '%.3f' % (p[0] * 1e3 / (steps * N)) if 'far' in name else '-'))
                sys.stdout.flush()
                stop = stop or p[0] > LIMIT_US
            env.set_state(desired=far)
            if N * 6 ** D <= 2 ** 27 and not stop:
                acts = strings(D, N)
                sim_out = env.simulate(acts)
                want = enumerated(env, D, acts, sim_out)
                got = env.plan(D, fields=KERNEL_FIELDS, out=out)
                assert all(torch.equal(got[f], want[f]) for f in KERNEL_FIELDS)                # (the two routes compute the same thing)
                p = timed(lambda: enumerated(env, D, acts, sim_out))
                print('%-7d %-3d %-12s %38s %12d %10s' % (N, D, 'enumerated', cell(p), D * 6 ** D, '-'))
                sys.stdout.flush()
                del acts, sim_out, want
                torch.cuda.empty_cache()
            if stop:
                print('# N = %d: a call above 2 s at D = %d, deeper calls not run' % (N, D))
                break
        env.close()


if __name__ == '__main__':
    main()
