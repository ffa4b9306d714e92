"""What "equal to the CPU oracle" means in the GPU tests, in one place.  An engine is built from known RNG states (make_env), its outputs and end
state are read into numpy arrays (record_steps, snapshot: the only parts that touch a GPU), and compared with the oracle either after the fact --
compare_with_oracle replays the recorded actions in slices of 8 192 envs on all host threads (cwo_batch_rollout); replay_against_oracle = snapshot +
compare_with_oracle -- or at the checkpoints of a test that steps an OracleBatch beside the engine (same_states, same_terminal).  Every comparison
covers every field it knows of every requested env, the RNG state exactly (key and position), and names the first envs that differ.  A plain
module, not a fixture; tests/test_oracle_replay_logic.py tests the comparisons themselves, on the CPU."""
import ctypes as C
import os

import numpy as np

SL = 8192
STATE = ('grid', 'init_grid', 'goal_grid', 'agent_rc', 'init_agent_rc', 'goal_agent_rc', 'hold', 'achieved', 'desired', 'step_num', 'ep_no')
FRAMES = {'observation': 'obs', 'desired_goal': 'desired_img', 'init_observation': 'init_img'}     # the engine's frame arrays: the oracle view's fields
VIEWS = ('render', 'grid_export', 'one_hot')                                                       # render(), grid() and one_hot() of the current state
OTHER = ('idx', 'rng_key', 'rng_pos', 'pool', 'terminal_observation')


def np_states(n, base):
    """numpy RandomState(base + i)'s (key, pos) for i < n"""
    sts = [np.random.RandomState(base + i).get_state() for i in range(n)]
    return np.stack([s[1] for s in sts]).astype(np.uint32), np.array([s[2] for s in sts], dtype=np.int32)


def oracle_kw(kw, raster='ray'):
    """the configuration `kw` as the oracle takes it: alt_obs=True is its name for CraftingWorldEnvAltObs's rasteriser"""
    return dict(kw, alt_obs=True) if raster == 'alt' else dict(kw)


def make_env(N, keys=None, pos=None, **kw):
    """The engine of a parity test and the RNG states its oracle starts from -> (env, keys, pos).  Given states are injected; without them they are
    the engine's own (seed=...).  fixed_init_state pools are drawn from the env streams at construction (ray.py:116-118): the pool is redrawn from
    (keys, pos), as the oracle draws its own."""
    from gym_craftingworld_amd import CraftingWorldVecEnv, _lib as L
    env = CraftingWorldVecEnv(N, **kw)
    given = keys is not None
    if not given:
        keys, pos = env.get_rng_states()
    if given or kw.get('fixed_init_state'):
        env.set_rng_states(keys, pos)
    if kw.get('fixed_init_state'):
        L.check(env._lib.cw_generate_fixed_states(env._h, env._stream()), 'pool')
    return env, keys, pos


def record_steps(env, actions):
    """env.step() through the device tensor `actions` [T, N] -> (rewards int32 [T, N], dones bool [T, N]), recorded on the device and read once"""
    import torch
    rs = torch.empty(actions.shape, dtype=torch.int32, device=actions.device)
    ds = torch.empty(actions.shape, dtype=torch.bool, device=actions.device)
    for t in range(actions.shape[0]):
        _, r, d, _ = env.step(actions[t])
        rs[t] = r
        ds[t] = d
    torch.cuda.synchronize()
    return rs.cpu().numpy(), ds.cpu().numpy()


def set_phase(ora, phase):
    """oracle env i's step_num := phase[i] and nothing else: the engine's set_state(step_num=phase)"""
    for e, p in zip(ora.envs, phase):
        v = e.view()
        e._lib.cwo_set_state(e._h, v.grid, v.init_grid, v.agent_r, v.agent_c, v.hold, v.achieved, v.desired, int(p))


def same(what, rows, got, want):
    """engine rows == oracle rows, else the first envs that differ; `rows`: the engine index of row 0, or of every row"""
    if not np.array_equal(got, want):
        if np.shape(got) != np.shape(want):
            raise AssertionError('%s: shape %s, the oracle has %s' % (what, np.shape(got), np.shape(want)))
        bad = np.nonzero((np.asarray(got) != np.asarray(want)).reshape(len(want), -1).any(axis=1))[0]
        rows = rows + np.arange(len(want)) if np.ndim(rows) == 0 else np.asarray(rows)
        raise AssertionError('%s differs from the oracle at %d envs, first %s' % (what, len(bad), rows[bad[:8]].tolist()))


def one_hot_of(grid, agent_rc, hold):
    """obs_one_hot (ray.py:94-98) of n states: channels 0-7 the objects, 8 the agent, 9-11 what it holds (at its cell) -> uint8 [n, S, S, 12]"""
    oh = np.zeros(grid.shape + (12,), np.uint8)
    for k in range(8):
        oh[..., k] = grid == k + 1
    r, a, h = np.arange(len(grid)), np.asarray(agent_rc, dtype=np.int64), np.asarray(hold, dtype=np.int64)
    oh[r, a[:, 0], a[:, 1], 8] = 1
    oh[r[h > 0], a[h > 0, 0], a[h > 0, 1], 8 + h[h > 0]] = 1
    return oh


def snapshot(env, idx=None, frames=(), terminal=False, pools=False, rng=True):
    """Everything a comparison needs from the engine, as numpy arrays, rows `idx` of the batch (default: all): get_state()'s fields, 'rng_key' and
    'rng_pos', the arrays named in `frames` (FRAMES: what step() returned last; VIEWS: render(), grid(), one_hot() now), 'terminal_observation',
    'pool' (the fixed_init_state pools) and 'idx' itself."""
    import torch
    idx = np.arange(env.num_envs) if idx is None else np.asarray(idx, dtype=np.int64)
    if idx.ndim != 1 or idx.size == 0 or idx.min() < 0 or idx.max() >= env.num_envs:
        raise ValueError('idx must select at least one env of the batch')
    if set(frames) - set(FRAMES) - set(VIEWS):
        raise ValueError('unknown frame arrays %s' % sorted(set(frames) - set(FRAMES) - set(VIEWS)))
    whole = len(idx) == env.num_envs and np.array_equal(idx, np.arange(env.num_envs))
    rows = None if whole else torch.as_tensor(idx, device=env.device)
    pick = lambda a: a if whole else a[idx]                       # noqa: E731
    host = lambda x: (x if whole else x[rows]).cpu().numpy()      # noqa: E731  (a sample is gathered on the device: only its rows are copied)
    snap = {k: pick(v) for k, v in env.get_state().items()}
    snap['idx'] = idx
    if rng:
        snap['rng_key'], snap['rng_pos'] = map(pick, env.get_rng_states())
    if pools:
        snap['pool'] = pick(env.fixed_states())
    views = {'render': env.render, 'grid_export': env.grid, 'one_hot': env.one_hot}
    for name in frames:
        snap[name] = host(env._observation()[name] if name in FRAMES else views[name]())
    if terminal:
        snap['terminal_observation'] = host(env.terminal_observation)
    return snap


def oracle_arrays(envs, names):
    """the oracle envs' side of a snapshot: the entries `names`, under the same names and in the same shapes"""
    views = [e.view() for e in envs]
    S, ish = envs[0].size, envs[0].img_shape

    def arr(field, shape):                                   # (one copy per env, straight into its row: this runs for every env of the full-size batches)
        a = np.empty((len(views),) + shape, np.uint8)
        base, size = a.ctypes.data, a[0].nbytes
        for j, v in enumerate(views):
            C.memmove(base + j * size, getattr(v, field), size)
        return a
    num = np.array([(v.agent_r, v.agent_c, v.init_agent_r, v.init_agent_c, v.goal_agent_r, v.goal_agent_c, v.hold, v.achieved, v.desired, v.step_num,
                     v.ep_no) for v in views], dtype=np.int64)
    out = dict(grid=arr('grid', (S, S)), init_grid=arr('init_grid', (S, S)), goal_grid=arr('goal_grid', (S, S)), agent_rc=num[:, 0:2],
               init_agent_rc=num[:, 2:4], goal_agent_rc=num[:, 4:6])
    out.update(zip(STATE[6:], num[:, 6:].T))
    for k in names:
        if k in FRAMES or k == 'render':
            out[k] = arr(FRAMES.get(k, 'obs'), ish)
    if 'grid_export' in names:
        out['grid_export'] = out['grid']
    if 'one_hot' in names:
        out['one_hot'] = one_hot_of(out['grid'], out['agent_rc'], out['hold'])
    if 'rng_key' in names:
        out.update(rng_key=np.empty((len(envs), 624), np.uint32), rng_pos=np.empty(len(envs), np.int32))
        kp, pp = out['rng_key'].ctypes.data, out['rng_pos'].ctypes.data
        for j, e in enumerate(envs):
            e._lib.cwo_get_rng(e._h, C.cast(kp + 2496 * j, C.POINTER(C.c_uint32)), C.cast(pp + 4 * j, C.POINTER(C.c_int32)))
    if 'pool' in names:
        out['pool'] = np.stack([e.fixed_states() for e in envs])
    return out


def _same_envs(snap, sl, envs, tag=''):
    """rows `sl` of the snapshot == these oracle envs, in everything the snapshot holds of an env (the terminal frames apart)"""
    if set(snap) - set(STATE) - set(FRAMES) - set(VIEWS) - set(OTHER):
        raise ValueError('unknown snapshot entries %s' % sorted(set(snap) - set(STATE) - set(FRAMES) - set(VIEWS) - set(OTHER)))
    want = oracle_arrays(envs, list(snap))
    assert set(want) == set(snap) - {'idx'}, sorted(set(want) ^ set(snap))      # (nothing the snapshot holds goes uncompared)
    for k in want:
        same(tag + k, snap['idx'][sl], snap[k][sl], want[k])


def compare_with_oracle(snap, keys, pos, kw, actions, rewards, dones, phase=None, per_env_kwargs=None):
    """Pure CPU.  `snap`: snapshot() of an engine that took T steps from the RNG states (keys, pos) and its reset, with `phase` (if given) set as
    every env's step_num right after that reset; `actions` int [T, N] (values 0..5), `rewards` / `dones` [T, N] what the engine returned on every
    step; `kw` the configuration as the oracle takes it, `per_env_kwargs` [N] what env i adds to it.  All of them span the whole batch; the oracle
    replays the rows snap['idx'].  Every reward and done, and at the end everything the snapshot holds ('terminal_observation': of the envs that
    finished on the last step).  -> dict(finished, successes, done_per_env [len(idx)]) of the oracle's run."""
    from oracle import OracleBatch
    if np.ndim(actions) != 2 or not np.shape(actions) == np.shape(rewards) == np.shape(dones):
        raise ValueError('actions %s, rewards %s and dones %s must be [T, N] alike' % (np.shape(actions), np.shape(rewards), np.shape(dones)))
    T, idx = actions.shape[0], snap['idx']
    a_host = np.asarray(actions, dtype=np.int8)
    terminal = 'terminal_observation' in snap
    last = T - 1 if terminal else T                          # (the last step in lock-step: the frame before the reset is the terminal one)
    threads = max(1, len(os.sched_getaffinity(0)))
    finished, successes = 0, 0
    done_per_env = np.zeros(len(idx), np.int64)
    for lo in range(0, len(idx), SL):
        sl = slice(lo, lo + SL)
        rows = idx[sl]
        ora = OracleBatch(len(rows), rng_states=[(keys[i], int(pos[i])) for i in rows],
                          per_env_kwargs=None if per_env_kwargs is None else [per_env_kwargs[i] for i in rows], **kw)
        ora.reset()
        if phase is not None:
            set_phase(ora, phase[rows])
        total, o_rew, o_done = ora.rollout(a_host[:last, rows], nthreads=threads, record=True)
        assert total == len(rows) * last
        o_done = o_done.astype(bool)
        if terminal:
            r_last, d_last, _, term = ora.step(a_host[T - 1, rows], details=True)
            o_rew, o_done = np.concatenate([o_rew, r_last[None]]), np.concatenate([o_done, d_last[None]])
            if term:
                same('terminal_observation', rows[d_last], snap['terminal_observation'][sl][d_last], np.stack([term[j] for j in sorted(term)]))
        same('reward of every step', rows, rewards[:, rows].T, o_rew.T)
        same('done of every step', rows, dones[:, rows].astype(bool).T, o_done.T)
        finished += int(o_done.sum())
        successes += int((o_rew == kw.get('max_steps', 300)).sum())
        done_per_env[sl] = o_done.sum(axis=0)
        _same_envs({k: v for k, v in snap.items() if k != 'terminal_observation'}, sl, ora.envs)
        del ora
    return dict(finished=finished, successes=successes, done_per_env=done_per_env)


def replay_against_oracle(env, keys, pos, kw, actions, rewards, dones, phase=None, frames=False, terminal=False, pools=False, per_env_kwargs=None,
                          idx=None):
    """snapshot(env) + compare_with_oracle.  frames: also the three frame arrays; terminal: also terminal_observation of the envs that finished on
    the last step; pools: also the fixed_init_state pools; idx: only these rows of the batch."""
    snap = snapshot(env, idx, tuple(FRAMES) if frames else (), terminal, pools)
    return compare_with_oracle(snap, keys, pos, kw, actions, rewards, dones, phase, per_env_kwargs)


def same_states(env_or_snapshot, ora, idx=None, frames=(), rng=True, tag=''):
    """For a test that steps `ora` (an OracleBatch) beside the engine: at this moment every get_state() field, the arrays named in `frames` (FRAMES,
    VIEWS) and, with rng, the RNG state of engine rows `idx` (default: all) == oracle envs 0 .. len(idx) - 1."""
    snap = env_or_snapshot if isinstance(env_or_snapshot, dict) else snapshot(env_or_snapshot, idx, frames, rng=rng)
    need = list(frames) + (['rng_key', 'rng_pos'] if rng else [])
    if [k for k in need if k not in snap]:
        raise ValueError('the snapshot does not hold %s' % [k for k in need if k not in snap])
    if len(snap['idx']) != len(ora.envs):
        raise ValueError('%d engine rows against %d oracle envs' % (len(snap['idx']), len(ora.envs)))
    _same_envs({k: v for k, v in snap.items() if k in STATE or k == 'idx' or k in need}, slice(None), ora.envs, tag)


def same_terminal(terminal_observation, o_term, idx=None, tag=''):
    """info['terminal_observation'] (device, [N, ...]) at the envs that just finished == the frames OracleBatch.step(details=True) kept of them before
    their reset (`o_term`: {oracle env: frame}); oracle env j is engine row idx[j]"""
    import torch
    if o_term:
        j = np.array(sorted(o_term))
        rows = j if idx is None else np.asarray(idx)[j]
        got = terminal_observation[torch.as_tensor(rows, device=terminal_observation.device)].cpu().numpy()
        same(tag + 'terminal_observation', rows, got, np.stack([o_term[i] for i in j]))


def assert_counters(env, N, T, res, invalid=0):
    """counters 0..3 of an engine that took T steps of N envs since it was created: env-steps, episodes finished, steps that returned max_steps,
    invalid actions"""
    c = env._counters_raw.cpu().numpy()
    assert (int(c[0]), int(c[1]), int(c[2]), int(c[3])) == (N * T, res['finished'], res['successes'], invalid), c
    return c
