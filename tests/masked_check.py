"""What "a masked call did exactly what it should" means for cw_imagine_masked / cw_sample_state_masked (and, for the rows a masked reset must leave alone,
cw_reset_masked), in one place.  take() reads an engine into numpy arrays -- the only part that touches a GPU -- and check_masked_call() compares a
snapshot taken before the call and one taken after it, the mask bytes, the desired words and what the call returned with the numpy model of
tests/imagine_model.py (pinned to the reference by tests/test_imagine_model.py and tests/test_imagine_sweep_model.py): EVERY selected row against the
model's result computed from the before-snapshot, every other row and buffer byte for byte against the before-snapshot.  A plain module, not a
fixture; tests/test_masked_shapes_logic.py tests the comparison itself, on the CPU.  Also here: the small helpers the GPU tests of these kernels share
(tests/test_imagine.py, tests/test_masked_shapes.py)."""
import numpy as np

import imagine_model as M
from oracle_replay import FRAMES, same

BUFFERS = ('hdr', 'slot_pos', 'reward', 'done', 'achieved_mask', 'desired_mask', 'episode_length', 'episode_return')
CW_WAVE, CW_RESET_WAVES = 64, 4


# ------------------------------------------------------------------------------------------------------------------------------ the launch rule
def masked_launch(n_envs, n_cu, reset_blocks=4):
    """the shape cwh_masked_launch (csrc/cw_host.h) gives the masked and snapshot kernels (CW_TUNE_RESET_BLOCKS) -> (epb, chunks, workgroups):
    a workgroup deals `epb` mask bytes a round -- 64, halved down to 4 while the chunks would not fill n_cu * reset_blocks workgroups"""
    most = n_cu * reset_blocks
    epb = CW_WAVE
    while epb > CW_RESET_WAVES and (n_envs + epb - 1) // epb < most:
        epb >>= 1
    chunks = (n_envs + epb - 1) // epb
    return epb, chunks, max(1, min(chunks, most))


# ------------------------------------------------------------------------------------------------------------------------------ the model, per row
def model_imagine(st, keys, pos, rows, desired):
    """imagine_obs of engine rows `rows` by the model, from get_state() `st` and the streams (keys, pos) -> (goal_grid [n,S,S], goal_agent_rc [n,2], the
    streams afterwards as numpy holds them)"""
    S = st['grid'].shape[1]
    g = np.zeros((len(rows), S, S), np.uint8)
    a = np.zeros((len(rows), 2), np.uint8)
    k2, p2 = np.empty((len(rows), 624), np.uint32), np.empty(len(rows), np.int32)
    rs = np.random.RandomState()
    for j, i in enumerate(rows):
        rs.set_state(('MT19937', keys[i], int(pos[i]), 0, 0.0))
        g[j], a[j] = M.imagine(st['init_grid'][i], st['init_agent_rc'][i], st['agent_rc'][i], int(desired[i]), rs)
        s = rs.get_state()
        k2[j], p2[j] = s[1], s[2]
    return g, a, k2, p2


def model_sample(size, keys, pos, rows, pool=None):
    """sample_state() (pool [N,K,9] given: generate_fixed_initial_state()) of rows `rows` -> (cells uint16 [n,9], the streams afterwards)"""
    want = np.empty((len(rows), 9), np.uint16)
    k2, p2 = np.empty((len(rows), 624), np.uint32), np.empty(len(rows), np.int32)
    rs = np.random.RandomState()
    for j, i in enumerate(rows):
        rs.set_state(('MT19937', keys[i], int(pos[i]), 0, 0.0))
        want[j] = M.sample_state(size, rs) if pool is None else M.generate_fixed_initial_state(pool[i], rs)
        s = rs.get_state()
        k2[j], p2[j] = s[1], s[2]
    return want, k2, p2


# ------------------------------------------------------------------------------------------------------------------------------ the engine's side
def device_side(env):
    """clones of every device buffer a masked call must leave alone in unselected rows"""
    out = {k: getattr(env, k).clone() for k in BUFFERS}
    out['counters'] = env._counters_raw.clone()
    if env.obs_mode != 'state':
        out.update({k: v.clone() for k, v in env._observation().items() if k != 'achieved_goal'})
    return out


def spread(env, T, seed, moves_only=False):
    """T random steps (+ reset_envs(done) on an auto_reset=False engine) -> the actions taken [T, N]"""
    import torch
    gen = torch.Generator(device='cuda').manual_seed(seed)
    acts = torch.randint(0, 4 if moves_only else 6, (T, env.num_envs), device='cuda', dtype=torch.uint8, generator=gen)
    for t in range(T):
        env.step(acts[t])
        if not env.auto_reset:
            env.reset_envs(env.done)
    torch.cuda.synchronize()
    return acts.cpu().numpy()


def take(env):
    """Everything check_masked_call compares, as numpy arrays: get_state()'s fields ('state_*'), the streams ('rng_key', 'rng_pos'), every buffer of
    BUFFERS (desired_mask as uint16), the raw counters and, in the pixel modes, the three frame arrays."""
    snap = {'state_' + k: v for k, v in env.get_state().items()}
    snap['rng_key'], snap['rng_pos'] = env.get_rng_states()
    for k in BUFFERS:
        snap[k] = getattr(env, k).cpu().numpy().copy()
    snap['desired_mask'] = snap['desired_mask'].view(np.uint16)
    snap['counters'] = env._counters_raw.cpu().numpy().copy()
    if env.obs_mode != 'state':
        for k in FRAMES:
            snap[k] = env._observation()[k].cpu().numpy().copy()
    return snap


# ------------------------------------------------------------------------------------------------------------------------------ the comparison
def _decode(oh):
    """one-hot states [n,S,S,12] -> (codes [n,S,S], agent (r, c) [n,2]: the first cell with channel 8 set)"""
    oh = np.asarray(oh)
    codes = (oh[..., :8].astype(np.int64) * np.arange(1, 9)).sum(axis=-1).astype(np.uint8)
    flat = oh[..., 8].reshape(len(oh), -1).argmax(axis=1)
    return codes, np.stack([flat // oh.shape[2], flat % oh.shape[2]], axis=1).astype(np.uint8)


def check_masked_call(kind, before, after, mask, *, desired=None, commit=False, frames=None, one_hot=None, cells=None, out_before=None, alt=False,
                      n_task_list=9, pool=None, allow_empty=False):
    """Pure CPU.  kind 'imagine': cw_imagine_masked(mask, desired, commit) ran between the snapshots `before` and `after` (take()) and returned
    `frames` [N, ...] and / or `one_hot` [N,S,S,12]; kind 'sample': cw_sample_state_masked(mask, pooled = pool is not None) returned `cells` [N,9]
    (`pool`: fixed_states(), [N,K,9]).  mask: the N bytes the kernel read (None: every env; any non-zero byte selects), desired: the N words it
    read (None: each env's own mask; bits at or above n_task_list are not used).  out_before: the output array as it stood before the call -- given,
    the rows of unselected envs must still hold it.
    Selected rows: goal grid and agent, frames (the oracle's rasterisers, alt=...), one-hot output, stream key and position and -- committed --
    get_state()'s goal_grid / goal_agent_rc / desired, desired_mask, hdr bytes 6-7 and the desired_goal frames equal the model's result from `before`.
    Everything else -- every other field of a selected row, every unselected row, the counters -- is byte-identical to `before`.
    Raises ValueError when asked to compare nothing: an empty selection without allow_empty=True.  -> the selected rows."""
    if kind not in ('imagine', 'sample'):
        raise ValueError('unknown kind %r' % (kind,))
    if set(before) != set(after):
        raise ValueError('the snapshots hold different entries: %s' % sorted(set(before) ^ set(after)))
    N = len(before['rng_pos'])
    mask = np.ones(N, np.uint8) if mask is None else np.asarray(mask).astype(np.uint8).reshape(-1)
    if len(mask) != N:
        raise ValueError('%d mask bytes for %d envs' % (len(mask), N))
    rows = np.flatnonzero(mask)
    if len(rows) == 0 and not allow_empty:
        raise ValueError('nothing selected: nothing would be compared with the model (allow_empty=True if that is the case under test)')
    outs = {'frames': frames, 'one_hot output': one_hot} if kind == 'imagine' else {'cells': cells}
    outs = {k: np.asarray(v) for k, v in outs.items() if v is not None}
    if not outs and not commit:
        raise ValueError('no output array and nothing committed: nothing of the result would be compared')
    st = {k[6:]: v for k, v in before.items() if k.startswith('state_')}
    want = dict(before)

    def patch(k, vals):
        want[k] = want[k].copy()
        want[k][rows] = vals

    if kind == 'imagine':
        if desired is None:
            used = st['desired'].astype(np.uint16)
        else:
            used = (np.asarray(desired).reshape(-1).astype(np.int64) & ((1 << n_task_list) - 1)).astype(np.uint16)
            if len(used) != N:
                raise ValueError('%d desired words for %d envs' % (len(used), N))
        g, a, k2, p2 = model_imagine(st, before['rng_key'], before['rng_pos'], rows, used)
        results = {}
        if 'one_hot output' in outs and len(rows):
            codes, agent = _decode(outs['one_hot output'][rows])
            same('goal grid', rows, codes, g)
            same('goal agent', rows, agent, a)
            results['one_hot output'] = np.stack([M.one_hot(g[j], a[j]) for j in range(len(rows))])
        if ('frames' in outs or (commit and 'desired_goal' in before)) and len(rows):
            img = np.stack([M.render(g[j], a[j], alt) for j in range(len(rows))])
            if 'frames' in outs:
                results['frames'] = img
        if commit and len(rows):
            patch('state_goal_grid', g)
            patch('state_goal_agent_rc', a)
            if 'desired_goal' in before:
                patch('desired_goal', img)
            if desired is not None:
                patch('state_desired', used[rows])
                patch('desired_mask', used[rows])
                want['hdr'] = want['hdr'].copy()
                want['hdr'][rows, 6], want['hdr'][rows, 7] = used[rows] & 0xFF, used[rows] >> 8
    else:
        S = st['grid'].shape[1]
        c, k2, p2 = model_sample(S, before['rng_key'], before['rng_pos'], rows, pool)
        results = {'cells': c} if len(rows) else {}
    if len(rows):
        patch('rng_key', k2)
        patch('rng_pos', p2)
    for k, got in outs.items():
        if k in results:
            same(k, rows, got[rows], results[k])
        if out_before is not None:
            rest = np.flatnonzero(mask == 0)
            same(k + ' of the unselected rows', rest, got[rest], np.asarray(out_before)[rest])
    for k in sorted(before):
        if k == 'counters':
            assert np.array_equal(after[k], before[k]), 'counters changed: %s -> %s' % (before[k].tolist(), after[k].tolist())
        else:
            same(k, 0, after[k], want[k])
    return rows


def untouched(before, after, mask, tag=''):
    """every entry of the rows with mask byte 0 is byte-identical in the two snapshots (the counters are the caller's: a masked reset on a look-ahead
    engine counts its slow resets) -> the unselected rows; an all-zero mask compares everything, the counters included"""
    rest = np.flatnonzero(np.asarray(mask).astype(np.uint8).reshape(-1) == 0)
    if len(rest) == 0:
        raise ValueError('every env is selected: nothing would be compared')
    assert set(before) == set(after)
    for k in sorted(before):
        if k == 'counters':
            if len(rest) == len(before['rng_pos']):
                assert np.array_equal(after[k], before[k]), tag + 'counters changed: %s -> %s' % (before[k].tolist(), after[k].tolist())
        else:
            same(tag + k + ' of the unselected rows', rest, after[k][rest], before[k][rest])
    return rest
