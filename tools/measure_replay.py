#!/usr/bin/env python3
"""Time the replay buffer's calls on one GPU beside the routes they replace -> the table of profiles/r15_replay.txt (stdout).

    python tools/measure_replay.py > profiles/r15_replay.txt

HIP events around single calls on the caller's stream (a call's launch gap is in the figure), medians (p10 .. p90) of 20 after a warm-up call, one process,
one build.  A state-only engine with auto-reset, 21x21, max_steps 300, 4 096 and 65 536 envs, a buffer of L = 256 steps filled by 2 L pushes of random
actions (so the ring has wrapped and slot order is position order).  "push": replay_push(actions).  "step": the state-only step() beside it, whose kernels
this change does not touch -- the parent commit's cost of a step.  "sample": replay_sample(B, her=0.8) of all thirteen fields into out= buffers, B = 4 096
and 65 536.  "sample + frames": the same plus the three render_records() calls that paint obs, next-obs and goal frames.  "torch route": the same minibatch
assembled in torch from replay_view() -- randint for env and position, index gathers of the six record arrays, the episode's last position from the
episode column, the future draw, the relabel with compute_reward_batch and the rewritten desired bytes."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from gym_craftingworld_amd import CraftingWorldVecEnv  # noqa: E402

STEPS, HER = 256, 0.8


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


def u16(h, at):
    return h[..., at].to(torch.int32) | h[..., at + 1].to(torch.int32) << 8


def torch_route(env, v, B, her):
    """the minibatch of replay_sample(B, her=her, strategy='future') assembled from the view (the buffer full and n a multiple of L: slot = position - lo)"""
    L, N = v['action'].shape
    i = torch.randint(0, N, (B,), device='cuda')
    p = torch.randint(0, L, (B,), device='cuda')
    relabel = torch.rand(B, device='cuda') < her
    ep = v['episode'][:, i]                                                     # [L, B]
    rows = torch.arange(L, device='cuda')[:, None]
    same = (ep == ep.gather(0, p[None])) & (rows >= p[None])
    e = torch.where(same, rows, 0).amax(0)
    f = p + (torch.rand(B, device='cuda') * (e - p + 1)).long().clamp_(max=L - 1)
    f = torch.minimum(f, e)
    out = {k: v[k][p, i].clone() for k in ('hdr', 'slot_pos', 'next_hdr', 'next_slot_pos', 'goal_hdr', 'goal_slot_pos', 'action', 'reward')}
    flags = v['flags'][p, i]
    at_f = v['next_hdr'][f, i]
    g = u16(at_f, 4)
    reward = env.compute_reward_batch(u16(out['next_hdr'], 4), g, subset=False)
    reward = torch.where((flags & 1) != 0, reward, torch.full_like(reward, -1))
    done = (u16(out['next_hdr'], 8) >= env.MAX_STEPS) | (reward == env.MAX_STEPS)
    gb = torch.stack([g & 255, g >> 8], 1).to(torch.uint8)
    for k in ('hdr', 'next_hdr'):
        out[k][:, 6:8] = torch.where(relabel[:, None], gb, out[k][:, 6:8])
    goal = at_f.clone()
    goal[:, 6:8] = gb
    out['goal_hdr'] = torch.where(relabel[:, None], goal, out['goal_hdr'])
    out['goal_slot_pos'] = torch.where(relabel[:, None], v['next_slot_pos'][f, i], out['goal_slot_pos'])
    out['reward'] = torch.where(relabel, reward, out['reward'])
    out['done'] = torch.where(relabel, done, (flags & 2) != 0)
    out['desired'] = torch.where(relabel, g, u16(v['hdr'][p, i], 6)).to(torch.int16)
    out['env'], out['slot'], out['future'] = i.to(torch.int32), p.to(torch.int32), torch.where(relabel, f, -1).to(torch.int32)
    return out


def frames(env, r):
    return (env.render_records(r['hdr'], r['slot_pos']), env.render_records(r['next_hdr'], r['next_slot_pos']),
            env.render_records(r['goal_hdr'], r['goal_slot_pos']))


def main():
    print('# the replay buffer (VecEnv.replay_push / replay_sample) on one %s: us per call, HIP events around single calls on the caller\'s stream (launch gap'
          % torch.cuda.get_device_name(0))
    print('# included), medians (p10 .. p90) of 20 calls after a warm-up call, one process.  obs_mode=state, auto-reset, 21x21, max_steps 300, N envs, L = %d' % STEPS)
    print('# steps, filled by 2 L pushes of random actions.  push: replay_push; step: the state-only step() beside it (kernels untouched by this change).  sample:')
    print('# replay_sample(B, her=%.1f), thirteen fields into out= buffers; torch route: the same minibatch from replay_view() with randint, index gathers, the' % HER)
    print('# episode end from the episode column and compute_reward_batch.  + frames: plus three render_records() calls (obs, next obs, goal).')
    print('# x: this row\'s median over that of the row above it (above 1: the new call is the faster one).')
    print('%-7s %-7s %-24s %38s %7s' % ('N', 'B', 'call', 'us per call', 'x'))
    for N in (4096, 65536):
        env = CraftingWorldVecEnv(N, size=(21, 21), max_steps=300, obs_mode='state', seed=3)
        env.reset()
        env.replay_reserve(STEPS)
        acts = torch.randint(0, 6, (2 * STEPS, N), device='cuda', dtype=torch.uint8)
        for t in range(2 * STEPS):
            env.replay_push(acts[t])
            env.step(acts[t])
        v = env.replay_view()

        def row(B, name, p, x=''):
            print('%-7d %-7s %-24s %38s %7s' % (N, B, name, cell(p), x))
            sys.stdout.flush()
        print('# N = %d: the buffer takes %.1f MiB' % (N, env.replay_bytes() / 2 ** 20))
        for B in (4096, 65536):
            out = env.replay_sample(B, 1, her=HER)
            p_s = timed(lambda: env.replay_sample(B, 1, her=HER, out=out))
            p_t = timed(lambda: torch_route(env, v, B, HER))
            row(B, 'sample', p_s)
            row(B, 'torch route', p_t, '%.2f' % (p_t[0] / p_s[0]))
            p_sf = timed(lambda: frames(env, env.replay_sample(B, 1, her=HER, out=out)))
            p_tf = timed(lambda: frames(env, torch_route(env, v, B, HER)))
            row(B, 'sample + frames', p_sf)
            row(B, 'torch route + frames', p_tf, '%.2f' % (p_tf[0] / p_sf[0]))
            del out
            torch.cuda.empty_cache()
        p_push = timed(lambda: env.replay_push(acts[0]))                        # (last: the pushes move n off the multiple of L the torch route reads)
        p_step = timed(lambda: env.step(acts[0]))
        row('-', 'push', p_push)
        row('-', 'step (state-only)', p_step, '%.2f' % (p_step[0] / p_push[0]))
        env.close()


if __name__ == '__main__':
    main()
