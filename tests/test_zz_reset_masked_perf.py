"""GPU tier, collected after tests/test_zz_perf_floors.py: the one timing relation of the partial reset.  What it computes is checked, bit-exact and without a
clock, in tests/test_reset_masked.py; under `pytest -x` a slow box can only lose this row."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_a_sparse_masked_reset_takes_at_most_half_of_a_full_reset():
    """65 536 envs, 21x21, full frames, auto_reset=False (the manual-reset use; its reset() carries no look-ahead refill, which would only make the
    yardstick slower).  reset() must write three frame arrays, 4.16 GB -- more than 0.52 ms at the card's 8 TB/s peak --, a reset_envs of 219 envs
    writes 219 x 3 frames = 13.9 MB and runs 219 independent one-wave resets: at most half the time, whatever the box.  Device events around single
    calls, alternating in one process, medians of 20 each after a warm-up of both."""
    from gym_craftingworld_amd import CraftingWorldVecEnv
    N = 65536
    env = CraftingWorldVecEnv(N, size=(21, 21), max_steps=300, obs_mode='pixels', auto_reset=False, seed=5)
    env.reset()
    sel = np.random.RandomState(1).choice(N, 219, replace=False)
    mask = torch.zeros(N, dtype=torch.bool, device=env.device)
    mask[torch.as_tensor(sel, device=env.device)] = True

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    for _ in range(3):
        timed(env.reset)
        timed(lambda: env.reset_envs(mask))
    full, part = [], []
    for _ in range(20):
        full.append(timed(env.reset))
        part.append(timed(lambda: env.reset_envs(mask)))
    full_ms, part_ms = float(np.median(full)), float(np.median(part))
    print('reset() %.3f ms, reset_envs(219 of %d) %.3f ms, ratio %.1f' % (full_ms, N, part_ms, full_ms / part_ms))
    assert part_ms <= 0.5 * full_ms, (part_ms, full_ms)
    env.close()
