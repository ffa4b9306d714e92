#!/usr/bin/env python3
"""Time cw_shoot_refit and one cem() iteration on one GPU beside the route they replace -> the table of profiles/r14_refit.txt (stdout).

    python tools/measure_refit.py > profiles/r14_refit.txt

HIP events around single calls on the caller's stream (a call's launch gap is in the figure), medians (p10 .. p90) of 20 after a warm-up call of every
shape, one process, one build.  A state-only engine, 21x21, max_steps 300, auto_reset=False, 4 096 and 65 536 envs ten random steps into their episodes;
(K samples, T steps, E elites) = (16, 8, 4), (64, 16, 8), (256, 32, 32), (1 024, 64, 64); uniform (no weights_in) and weighted (uint16 [T, 6, N], refitted
in place).  "refit": shoot_refit() of the returns a shoot() call left, all three fields into out= buffers.  "torch route": what a caller wrote before the
call existed -- torch.topk over dim 0 (its tie order unspecified), shoot_actions(samples=elites) into a [T, E, N] buffer, a scatter_add histogram, and
smooth + gain * counts clamped and cast to uint16 -- the same returns, seed and weights.  "cem, 1 iteration": cem(iters=1) with out=, i.e. shoot() and the
refit; "shoot + torch route": the same iteration with the torch route in the refit's place."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from gym_craftingworld_amd import CraftingWorldVecEnv  # noqa: E402
from gym_craftingworld_amd.vec_env import SHOOT_FIELDS  # noqa: E402

DEFAULT = tuple(f for f in SHOOT_FIELDS if f not in ('hdr', 'slot_pos', 'ret'))
SHAPES = ((16, 8, 4), (64, 16, 8), (256, 32, 32), (1024, 64, 64))
SMOOTH, GAIN = 1, 16


def timed(fn):
    """one warm-up call, then 20 timed ones -> (p50, p10, p90) in us"""
    def once():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3
    once()
    return np.percentile([once() for _ in range(20)], [50, 10, 90])


def cell(p):
    return '%11.1f (%10.1f..%10.1f)' % tuple(p)


def to_uint16(x):
    try:
        return x.to(torch.uint16)
    except (RuntimeError, TypeError):          # (a torch without that cast: the same bits through int16)
        return x.to(torch.int16).view(torch.uint16)


def torch_route(env, ret, T, E, seed, w, acts, ones):
    top = torch.topk(ret, E, dim=0).indices.to(torch.int32)
    a = env.shoot_actions(T, seed, samples=top, weights=w, out=acts)
    hist = torch.zeros((T, 6, ret.shape[1]), dtype=torch.int32, device='cuda')
    hist.scatter_add_(1, a.to(torch.int64), ones)
    return to_uint16((SMOOTH + GAIN * hist).clamp_(max=65535))


def main():
    print('# cw_shoot_refit (VecEnv.shoot_refit) and one cem() iteration on one %s: us per call, HIP events around single calls on the caller\'s stream (launch'
          % torch.cuda.get_device_name(0))
    print('# gap included), medians (p10 .. p90) of 20 calls after a warm-up call, one process.  obs_mode=state, 21x21, max_steps 300, auto_reset=False, N envs ten')
    print('# random steps in; K samples, T steps, E elites; smooth %d, gain %d.  uniform: no weights_in; weighted: uint16 weights [T, 6, N], refitted in place.' % (SMOOTH, GAIN))
    print('# refit: shoot_refit of shoot()\'s returns, all three fields into out= buffers.  torch route: topk(dim 0) + shoot_actions(samples=elites) + scatter_add')
    print('# histogram + clamp + cast to uint16.  cem, 1 iteration: cem(iters=1, out=...), shoot() and the refit.  shoot + torch route: the same with the torch route')
    print('# in the refit\'s place.  x: this row\'s median over that of the row above it (above 1: the new call is the faster one).')
    print('%-7s %-5s %-3s %-3s %-9s %-20s %38s %7s' % ('N', 'K', 'T', 'E', 'draw', 'call', 'us per call', 'x'))
    for N in (4096, 65536):
        env = CraftingWorldVecEnv(N, size=(21, 21), max_steps=300, obs_mode='state', auto_reset=False, seed=3)
        env.reset()
        warm = torch.randint(0, 6, (10, N), device='cuda', dtype=torch.uint8)
        for t in range(10):
            env.step(warm[t])
        for K, T, E in SHAPES:
            for draw in ('uniform', 'weighted'):
                w0 = torch.randint(1, 20000, (T, 6, N), device='cuda', dtype=torch.int16).view(torch.uint16) if draw == 'weighted' else None
                w = None if w0 is None else w0.clone()
                shot = env.shoot(T, K, 1, weights=w, fields=DEFAULT + ('ret',))
                ret = shot['ret']
                fit = env.shoot_refit(ret, E, T, 1, weights=w, smooth=SMOOTH, gain=GAIN)
                if w is not None:
                    fit['weights'] = w                                           # in place
                acts = torch.empty((T, E, N), dtype=torch.uint8, device='cuda')
                ones = torch.ones((), dtype=torch.int32, device='cuda').expand(T, E, N)
                loop = env.cem(T, K, E, 1, 1, weights=w0, smooth=SMOOTH, gain=GAIN)

                def row(name, p, x=''):
                    print('%-7d %-5d %-3d %-3d %-9s %-20s %38s %7s' % (N, K, T, E, draw, name, cell(p), x))
                    sys.stdout.flush()

                def shoot_then_route():
                    env.shoot(T, K, 1, weights=w0, fields=DEFAULT + ('ret',), out=shot)
                    torch_route(env, ret, T, E, 1, w0, acts, ones)
                p_fit = timed(lambda: env.shoot_refit(ret, E, T, 1, weights=w, smooth=SMOOTH, gain=GAIN, out=fit))
                p_route = timed(lambda: torch_route(env, ret, T, E, 1, w0, acts, ones))
                row('refit', p_fit)
                row('torch route', p_route, '%.2f' % (p_route[0] / p_fit[0]))
                p_cem = timed(lambda: env.cem(T, K, E, 1, 1, weights=None if w0 is None else loop['weights'], smooth=SMOOTH, gain=GAIN, out=loop))
                p_both = timed(shoot_then_route)
                row('cem, 1 iteration', p_cem)
                row('shoot + torch route', p_both, '%.2f' % (p_both[0] / p_cem[0]))
                del shot, ret, fit, acts, ones, loop, w, w0
                torch.cuda.empty_cache()
        env.close()


if __name__ == '__main__':
    main()
