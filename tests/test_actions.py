"""GPU test: actions of every dtype and value.  A value outside 0..5 is the counted no-op (step_num + 1, reward -1, counters[3]; craftingworld.h)
whatever its dtype: an int64 beyond the int range is not cut down to its low 32 bits, and rollout() and a host_outputs engine do not wrap an int64
into 0..5 on the way to their uint8 / int32 buffers.  The same batch driven through step(), step_many(), rollout() and a host_outputs engine must
give the same rewards, dones, state, counters and RNG streams as step() with the out-of-range values written as -1 (int32) or 255 (uint8)."""
import numpy as np
import pytest
import torch

from oracle_replay import replay_against_oracle

pytestmark = pytest.mark.gpu

ODD = [6, 255, 256 + 2, 2 ** 31 - 1, 2 ** 31, 2 ** 32 + 2, -1, -2 ** 32 + 3, 2 ** 63 - 1, -2 ** 63]


def _table(T, N):
    rng = np.random.RandomState(11)
    a = rng.randint(0, 6, size=(T, N)).astype(np.int64)
    odd = rng.rand(T, N) < 0.25
    a[odd] = np.array(ODD, dtype=np.int64)[rng.randint(0, len(ODD), size=int(odd.sum()))]
    return a


def test_actions_of_every_dtype_and_value_are_the_same_steps():
    """a [T, N] int64 table mixing 0..5 with ODD through six paths; the reference is step() with int32 actions, every odd value written as -1"""
    from gym_craftingworld_amd import CraftingWorldVecEnv
    N, T = 3001, 64
    kw = dict(size=(6, 6), max_steps=9)
    a64 = _table(T, N)
    valid = (a64 >= 0) & (a64 <= 5)
    assert set(np.unique(a64[~valid]).tolist()) == set(ODD)
    a32 = np.where(valid, a64, -1).astype(np.int32)
    a8 = np.where(valid, a64, 255).astype(np.uint8)

    def engine(**extra):
        e = CraftingWorldVecEnv(N, obs_mode='state', seed=99, **kw, **extra)
        e.reset()
        return e

    def stepped(actions):
        e = engine()
        rs, ds = [], []
        for t in range(T):
            _, r, d, _ = e.step(actions[t])
            rs.append(r.cpu())
            ds.append(d.cpu())
        return e, torch.stack(rs), torch.stack(ds)

    runs = {}
    d64 = torch.as_tensor(a64, device='cuda')
    runs['step int32'] = stepped(torch.as_tensor(a32, device='cuda'))
    runs['step uint8'] = stepped(torch.as_tensor(a8, device='cuda'))
    runs['step int64'] = stepped(d64)
    e = engine()
    e.step_many(d64)
    runs['step_many int64'] = (e, None, None)
    e = engine()
    rew, don = e.rollout(d64)
    runs['rollout int64'] = (e, rew.cpu(), don.cpu())
    e = engine(host_outputs=True)
    rs, ds = [], []
    for t in range(T):
        _, r, d, _ = e.step(a64[t])                          # (a numpy int64 array: the engine's mapped int32 buffer)
        rs.append(r.clone())
        ds.append(d.clone())
    runs['host_outputs numpy int64'] = (e, torch.stack(rs).cpu(), torch.stack(ds).cpu())

    ref, r_ref, d_ref = runs['step int32']
    torch.cuda.synchronize()
    st_ref, (k_ref, p_ref) = ref.get_state(), ref.get_rng_states()
    assert int(ref.counters[3]) == int((~valid).sum()) and int(ref.counters[1]) >= N
    bad = []                                                 # (every path that differs, and in what: not only the first)
    for name, (e, r, d) in runs.items():
        if r is not None and not (torch.equal(r, r_ref) and torch.equal(d, d_ref)):
            bad.append((name, 'rewards / dones of the steps'))
        for k in ('reward', 'done', 'achieved_mask', 'desired_mask', 'episode_length', 'episode_return', 'counters'):
            if not torch.equal(getattr(e, k).cpu(), getattr(ref, k).cpu()):
                bad.append((name, k))
        st = e.get_state()
        bad += [(name, k) for k in st if not np.array_equal(st[k], st_ref[k])]
        k2, p2 = e.get_rng_states()
        if not (np.array_equal(p2, p_ref) and np.array_equal(k2, k_ref)):
            bad.append((name, 'rng'))
    assert not bad, bad
    for e, _, _ in runs.values():
        e.close()


def test_valid_actions_of_every_dtype_against_the_oracle():
    """random actions 0..5 in int64, int32 and uint8 tensors: each engine against the oracle"""
    from gym_craftingworld_amd import CraftingWorldVecEnv
    N, T = 2053, 40
    kw = dict(size=(6, 6), max_steps=9)
    a = np.random.RandomState(5).randint(0, 6, size=(T, N))
    for dt in (torch.int64, torch.int32, torch.uint8):
        e = CraftingWorldVecEnv(N, obs_mode='state', seed=7, **kw)
        keys, pos = e.get_rng_states()
        e.reset()
        acts = torch.as_tensor(a, device='cuda').to(dt)
        rs, ds = [], []
        for t in range(T):
            _, r, d, _ = e.step(acts[t])
            rs.append(r.cpu())
            ds.append(d.cpu())
        replay_against_oracle(e, keys, pos, kw, a, torch.stack(rs).numpy(), torch.stack(ds).numpy())
        e.close()
