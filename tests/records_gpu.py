"""What the GPU tiers of the records calls (tests/test_{expand,simulate,plan,shoot}.py) share: sentinel-filled output buffers built from the layouts of the
check modules, results as numpy, the env_of cases, goals within reach, records of the caller's, and the 70-env engine they hand in; and what the two GPU
tiers of cw_reach (tests/test_reach_async.py, tests/test_reach_rounds.py) share: its sentinel-filled outputs and start rows tiled from an engine's envs.
Imports torch: only `gpu` tests import it.  A plain module, not a fixture."""
import numpy as np
import torch

from engines import K5, N1
from masked_check import spread
from oracle_replay import make_env, np_states
from records_check import RECORD

SENT = 0xA5
INT32_MAX = 2 ** 31 - 1


def sentinel_out(layout, widths, dtypes, M):
    """output buffers as a records call's out= takes them, every byte SENT: field f of `layout` ({field: prefix shape}, as records_check.check_records_call
    reads it) is layout[f] + [M] rows of widths[f] bytes, seen as dtypes[f]"""
    out = {}
    for f, prefix in layout.items():
        t = torch.full(tuple(prefix) + (M, widths[f]), SENT, dtype=torch.uint8, device='cuda').view(dtypes[f])
        out[f] = t if f in RECORD else t.squeeze(-1)
        assert out[f].is_contiguous() and tuple(out[f].shape[:len(prefix) + 1]) == tuple(prefix) + (M,)
    return out


def host(result, fields=None):
    """a records call's result as numpy (the entries named in `fields`: all), bool fields as the bytes the kernel wrote"""
    return {f: (t.view(torch.uint8) if t.dtype is torch.bool else t).cpu().numpy() for f, t in result.items() if fields is None or f in fields}


def dev(a, dtype=np.uint8):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device='cuda')


def env_of_cases(M, N):
    """M entries: random envs (repeats), and from 63 states on -1, -7, N, N + 31 and INT32_MAX, the wave's last lane among their places"""
    e = np.random.RandomState(M).randint(0, N, M).astype(np.int64)
    if M >= 63:
        e[[3, 17, 31, 40, 62]] = [-1, N, -7, N + 31, INT32_MAX]
        e[5] = e[6] = e[7]
    if M >= 257:
        e[[63, 64, 128, 255, 256]] = [N, -1, INT32_MAX, N + 31, N]
    return e


def walk_goals(env, steps, seed, every=2):
    """desired of every `every`-th env := the achieved mask it reaches after `steps` steps of a random walk (simulate(), no env touched): goals within reach"""
    walk = dev(np.random.RandomState(seed).randint(0, 6, (steps, env.num_envs)))
    reached = env.simulate(walk, stop_at_done=False)['achieved_mask'].cpu().numpy().view(np.uint16)
    des = env.get_state()['desired'].astype(np.uint16)
    des[::every] = reached[::every]
    env.set_state(desired=des)


def caller_records(before, e, M, n_envs, max_steps):
    """M records of the caller's from the snapshot `before`: record j is env e[j]'s own (env 0's where e[j] names none) -> hdr, slot_pos"""
    src = np.where((e >= 0) & (e < n_envs), e, 0)
    hdr = before['hdr'][src].copy()
    hdr[:, 8] = (hdr[:, 8] + np.arange(M)) % max_steps                            # other step counts than the envs' own
    hdr[:, 3] = np.arange(M) % 5                                                  # ... and menu bytes, which every records call keeps
    return hdr, before['slot_pos'][src].copy()


def walked_engine(seed, steps, goals=None):
    """a 70-env engine on 5 x 5 without auto-reset, `steps` random steps into its episodes; goals: (steps, seed) of walk_goals.  The caller closes it."""
    env, _, _ = make_env(N1, *np_states(N1, seed), obs_mode='state', auto_reset=False, **K5)
    env.reset()
    spread(env, steps, 3)
    if goals:
        walk_goals(env, *goals)
    return env


# ------------------------------------------------------------------------------------------------------------------------------ cw_reach
REACH_OUT = (('distance', torch.int32), ('plan', torch.uint8), ('first_action', torch.uint8), ('frontier', torch.int32), ('searched_depth', torch.int32))


def reach_sentinel_out(D, M0):
    """the five output buffers of reach_async(D, M0 start rows, out=...), every byte SENT"""
    shapes = dict(distance=(M0,), plan=(D, M0), first_action=(M0,), frontier=(D,), searched_depth=(1,))
    return {f: torch.full(shapes[f] + (dt.itemsize,), SENT, dtype=torch.uint8, device='cuda').view(dt).squeeze(-1) for f, dt in REACH_OUT}


def tiled_rows(env, M0):
    """M0 start rows tiled from the engine's envs: row j is env j % N's state"""
    e = np.arange(M0) % env.num_envs
    return dev(env.hdr.cpu().numpy()[e]).reshape(M0, 16), dev(env.slot_pos.cpu().numpy()[e], np.int16).reshape(M0, 8), dev(e, np.int32)
