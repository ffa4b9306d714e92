#!/usr/bin/env python3
"""Time cw_shoot on one GPU beside the route it replaces -> the table of profiles/r11_shoot.txt (stdout).

    python tools/measure_shoot.py > profiles/r11_shoot.txt

HIP events around single calls on the caller's stream (a call's launch gap is in the figure), medians (p10 .. p90) after a warm-up call of every shape,
one process, one build.  A state-only engine, 21x21, max_steps 300, auto_reset=False, 4 096 and 65 536 envs ten random steps into their episodes; K = 16,
64, 256, 1 024 samples x T = 8, 16, 32, 64 steps, all under the cap of 2^32 steps a call.  "far": the goals reset() drew, out of reach within the horizon
-- no sample ends, every one of the K x T steps of a state is taken: the worst case.  "near": every env's goal is the achieved mask three random steps
reach, so that some samples end early.  "+ret": the far call with the [K, N] returns written as well.  "weights": the far call with per-state uint16
weights [T, 6, N] (the weighted instance of the kernel).  "randint+simulate": the same default results by the route that existed before -- torch.randint(0,
6, (T, K, N), dtype=uint8) INSIDE the timing (generating the actions is what the kernel removes), simulate() of the envs' own states broadcast over the K
plans, and the reduction and gather in torch (maximum, smallest maximiser, its rows and its plan)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from gym_craftingworld_amd import CraftingWorldVecEnv  # noqa: E402
from gym_craftingworld_amd.vec_env import SHOOT_FIELDS  # noqa: E402

DEFAULT = tuple(f for f in SHOOT_FIELDS if f not in ('hdr', 'slot_pos', 'ret'))
SIM_FIELDS = ('ret', 'length', 'done', 'achieved_mask')
CAP = 2 ** 32


def timed(fn):
    """one warm-up call, then 20 timed ones (5 above 10 ms a call) -> (p50, p10, p90) in us"""
    def once():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3
    first = once()
    out = [once() for _ in range(20 if first < 1e4 else 5)]
    return np.percentile(out, [50, 10, 90])


def cell(p):
    return '%11.1f (%10.1f..%10.1f)' % tuple(p)


def parent_route(env, T, K, sim_out, ks, cols):
    N = env.num_envs
    acts = torch.randint(0, 6, (T, K, N), dtype=torch.uint8, device='cuda')
    r = env.simulate(acts, fields=SIM_FIELDS, out=sim_out)
    ret = r['ret'].view(K, N)
    best = ret.amax(dim=0)
    first = torch.where(ret == best[None], ks, K).amin(dim=0)
    flat = first * N + cols
    out = {f: r[f][flat] for f in SIM_FIELDS[1:]}
    out['plan'] = acts[:, first, cols]
    out.update(best_ret=best, best_sample=first, best_action=out['plan'][0])
    return out


def main():
    print('# cw_shoot (VecEnv.shoot) on one %s: us per call, HIP events around single calls on the caller\'s stream (launch gap included), medians (p10 .. p90)'
          % torch.cuda.get_device_name(0))
    print('# of 20 calls (5 above 10 ms) after a warm-up call, one process.  obs_mode=state, 21x21, max_steps 300, auto_reset=False, N envs ten random steps in,')
    print('# the default fields into out= buffers.  far: no goal within the horizon, all K x T steps of a state are taken; near: goals three random steps away;')
    print('# +ret: far, with ret [K, N]; weights: far, uint16 weights [T, 6, N]; randint+simulate: torch.randint(0, 6, (T, K, N), uint8) + simulate() of the K x N')
    print('# plans + the torch reduction and gather, goals far, the generation inside the timing.  ns/step: the far figure per state-sample-step; x: the route\'s')
    print('# median over the far call\'s.')
    print('%-7s %-5s %-3s %-17s %38s %9s %7s' % ('N', 'K', 'T', 'call', 'us per call', 'ns/step', 'x'))
    for N in (4096, 65536):
        env = CraftingWorldVecEnv(N, size=(21, 21), max_steps=300, obs_mode='state', auto_reset=False, seed=3)
        env.reset()
        warm = torch.randint(0, 6, (10, N), device='cuda', dtype=torch.uint8)
        for t in range(10):
            env.step(warm[t])
        far = env.get_state()['desired'].astype(np.uint16)
        near = env.simulate(torch.randint(0, 6, (3, N), device='cuda', dtype=torch.uint8), stop_at_done=False)['achieved_mask'].cpu().numpy().view(np.uint16)
        cols = torch.arange(N, device='cuda')
        for K in (16, 64, 256, 1024):
            ks = torch.arange(K, device='cuda')[:, None]
            for T in (8, 16, 32, 64):
                if N * K * T > CAP:
                    continue
                out = env.shoot(T, K, 1, fields=DEFAULT)
                with_ret = env.shoot(T, K, 1, fields=DEFAULT + ('ret',))
                w = torch.randint(-32768, 32768, (T, 6, N), device='cuda', dtype=torch.int16).view(torch.uint16)

                def row(name, p, extra='', x=''):
                    print('%-7d %-5d %-3d %-17s %38s %9s %7s' % (N, K, T, name, cell(p), extra, x))
                    sys.stdout.flush()
                env.set_state(desired=near)
                p_near = timed(lambda: env.shoot(T, K, 1, fields=DEFAULT, out=out))
                env.set_state(desired=far)
                p_far = timed(lambda: env.shoot(T, K, 1, fields=DEFAULT, out=out))
                row('shoot, far', p_far, '%.4f' % (p_far[0] * 1e3 / (N * K * T)))
                row('shoot, near', p_near)
                row('shoot, far +ret', timed(lambda: env.shoot(T, K, 1, fields=DEFAULT + ('ret',), out=with_ret)))
                row('shoot, weights', timed(lambda: env.shoot(T, K, 1, weights=w, fields=DEFAULT, out=out)))
                sim_out = env.simulate(torch.zeros((T, K, N), dtype=torch.uint8, device='cuda'), fields=SIM_FIELDS)
                p = timed(lambda: parent_route(env, T, K, sim_out, ks, cols))
                row('randint+simulate', p, '', '%.1f' % (p[0] / p_far[0]))
                del sim_out, with_ret, out, w
                torch.cuda.empty_cache()
        env.close()


if __name__ == '__main__':
    main()
