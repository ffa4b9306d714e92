#!/usr/bin/env python3
"""Time cw_render_records on one GPU beside the path it replaces -> the table of profiles/r09_render_records.txt (stdout).

    python tools/measure_render_records.py > profiles/r09_render_records.txt

HIP events around single calls on the caller's stream (a call's launch gap is in the figure), medians (p10 .. p90) of 100 calls after a warm-up, one
process, one build.  A state-only engine, 21x21, auto_reset=False, in both rasters, at 4 096 and 65 536 envs: the records are the 6 N successors of
expand() (M is capped where the buffers of the old path would not fit in half the free device memory; the table says what M was).  "the two-kernel
path": the same frames through the calls that existed before -- one_hot_states() + render_states() + .to(torch.uint8).  "fill": torch.Tensor.fill_ on
the output array, the ceiling of anything that writes those bytes.  "render(), unaligned": cw_render of the N envs into an array the sweep cannot take,
which goes through the same painter of single frames (cw_render_frames_kernel)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from gym_craftingworld_amd import CraftingWorldVecEnv  # noqa: E402

CALLS = 100


def timed(fn, n=CALLS, warm=3):
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
    sizes = (4096, 65536)
    print('# cw_render_records (VecEnv.render_records) on one %s: us per call, HIP events around single calls on the caller\'s stream (launch gap included),'
          % torch.cuda.get_device_name(0))
    print('# medians (p10 .. p90) of %d calls after a warm-up of every shape, one process.  obs_mode=state, 21x21, max_steps 300, auto_reset=False.' % CALLS)
    print('# The records: the 6 N successors of expand() after 10 random steps (M states, below).  "mask=changed": expand()\'s changed bytes as the mask;')
    print('# "the two-kernel path": one_hot_states(out=...) + render_states() + .to(torch.uint8) on the same records; "fill": fill_(0) on the M output frames;')
    print('# "render(), unaligned": cw_render of the N envs through cw_render_frames_kernel (N frames, not M).  TB/s: bytes of the frames written / median.')
    for raster in ('ray', 'alt'):
        rows, notes, tbs = {}, [], {}
        for N in sizes:
            env = CraftingWorldVecEnv(N, size=(21, 21), max_steps=300, obs_mode='state', auto_reset=False, seed=3, raster=raster)
            env.reset()
            acts = torch.randint(0, 6, (10, N), device='cuda', dtype=torch.uint8)
            for t in range(10):
                env.step(acts[t])
            r = env.expand()
            fb = int(np.prod(env.frame_shape))
            per_state = 5 * fb + 12 * 21 * 21 + 64                 # out, the int16 image, its uint8 copy, the one-hot scratch, the records
            M = min(6 * N, int(torch.cuda.mem_get_info()[0] // 2 // per_state))
            hdr, pos = r['hdr'].reshape(-1, 16)[:M].contiguous(), r['slot_pos'].reshape(-1, 8)[:M].contiguous()
            changed = r['changed'].reshape(-1)[:M].contiguous()
            share = float(changed.float().mean())
            out = torch.empty((M,) + tuple(env.frame_shape), dtype=torch.uint8, device='cuda')
            oh = torch.empty((M, 21, 21, 12), dtype=torch.uint8, device='cuda')
            odd = torch.empty(N * fb + 16, dtype=torch.uint8, device='cuda')[4:4 + N * fb].view((N,) + tuple(env.frame_shape))
            notes.append('%d envs: M = %d states (%s), %.2f GB of frames, %.0f %% of them changed' %
                         (N, M, '6 N' if M == 6 * N else 'capped', M * fb / 1e9, 100 * share))
            calls = [('render_records', lambda: env.render_records(hdr, pos, out=out), M * fb),
                     ('render_records, mask=changed', lambda: env.render_records(hdr, pos, mask=changed, out=out), share * M * fb),
                     ('the two-kernel path', lambda: env.render_states(env.one_hot_states(hdr, pos, out=oh)).to(torch.uint8), M * fb),
                     ('fill', lambda: out.fill_(0), M * fb),
                     ('render(), unaligned', lambda: env.render(out=odd), N * fb)]
            for name, fn, nbytes in calls:
                p = timed(fn)
                rows.setdefault(name, []).append(p)
                tbs.setdefault(name, []).append(nbytes / (p[0] * 1e-6) / 1e12)
            env.close()
            del env, out, oh, odd, r, hdr, pos, changed
            torch.cuda.empty_cache()
        print('# raster=%s: %s' % (raster, '; '.join(notes)))
        print('%-30s %32s %32s %16s' % ('call', '%d envs' % sizes[0], '%d envs' % sizes[1], 'TB/s'))
        for name, r in rows.items():
            print('%-30s %32s %32s %7.2f %7.2f' % (name, cell(r[0]), cell(r[1]), tbs[name][0], tbs[name][1]))


if __name__ == '__main__':
    main()
