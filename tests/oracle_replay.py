"""The GPU tests' replay of a whole batch through the CPU oracle: the engine has run T steps of recorded actions; the oracle replays the same
actions in slices of 8 192 envs on all host threads (cwo_batch_rollout) and every reward and done of every step, and at the end every env's state,
frames and RNG state (key and position, exactly), must be the engine's.  A plain module, not a fixture: tests/test_launch_shapes.py and
tests/test_actions.py call it."""
import os

import numpy as np

SL = 8192


def np_states(n, base):
    """numpy RandomState(base + i)'s (key, pos) for i < n"""
    sts = [np.random.RandomState(base + i).get_state() for i in range(n)]
    return np.stack([s[1] for s in sts]).astype(np.uint32), np.array([s[2] for s in sts], dtype=np.int32)


def same(what, lo, got, want):
    """engine rows == oracle rows, else the first envs that differ"""
    if not np.array_equal(got, want):
        bad = np.nonzero((np.asarray(got) != np.asarray(want)).reshape(len(want), -1).any(axis=1))[0]
        raise AssertionError('%s differs from the oracle at %d envs, first %s' % (what, len(bad), (lo + bad[:8]).tolist()))


def replay_against_oracle(env, keys, pos, kw, actions, rewards, dones, phase=None, frames=False, terminal=False, pools=False):
    """`env` after T steps from the RNG states (keys, pos) and its reset, with `phase` (if given) set as every env's step_num right after that reset;
    `actions` int [T, N] (values 0..5), `rewards` / `dones` [T, N] what the engine returned on every step (host arrays); `kw` the env's
    configuration as the oracle takes it.  frames: also the three frame arrays; terminal: also terminal_observation of the envs that finished on the
    last step; pools: also the fixed_init_state pools.  -> dict(finished, successes, done_per_env [N]) of the oracle's run."""
    from oracle import OracleBatch
    N, T = env.num_envs, actions.shape[0]
    a_host = np.ascontiguousarray(actions, dtype=np.int8)
    st = env.get_state()
    k2, p2 = env.get_rng_states()
    pool = env.fixed_states() if pools else None
    obs = env._observation() if (frames or terminal) else None
    threads = max(1, len(os.sched_getaffinity(0)))
    finished, successes = 0, 0
    done_per_env = np.zeros(N, np.int64)
    for lo in range(0, N, SL):
        hi = min(N, lo + SL)
        n = hi - lo
        ora = OracleBatch(n, rng_states=[(keys[i], int(pos[i])) for i in range(lo, hi)], **kw)
        if pools:
            for j, e in enumerate(ora.envs):
                assert np.array_equal(pool[lo + j], e.fixed_states()), ('fixed_init_state pool', lo + j)
        ora.reset()
        if phase is not None:
            for j, e in enumerate(ora.envs):                 # the same phase spread (step_num only)
                v = e.view()
                e._lib.cwo_set_state(e._h, v.grid, v.init_grid, v.agent_r, v.agent_c, v.hold, v.achieved, v.desired, int(phase[lo + j]))
        last = T - 1 if terminal else T                      # (the last step one env at a time: the frame before the reset is the terminal one)
        total, o_rew, o_done = ora.rollout(a_host[:last, lo:hi], nthreads=threads, record=True)
        assert total == n * last
        o_done = o_done.astype(bool)
        if terminal:
            term = env.terminal_observation[lo:hi].cpu().numpy()
            r_last, d_last = np.empty(n, np.int32), np.zeros(n, bool)
            for j, e in enumerate(ora.envs):
                o, r_last[j], d_last[j], _ = e.step(int(a_host[T - 1, lo + j]))
                if d_last[j]:
                    assert np.array_equal(term[j], o['observation']), ('terminal_observation', lo + j)
                    e.reset()
            o_rew, o_done = np.concatenate([o_rew, r_last[None]]), np.concatenate([o_done, d_last[None]])
        same('reward of every step', lo, rewards[:, lo:hi].T, o_rew.T)
        same('done of every step', lo, dones[:, lo:hi].astype(bool).T, o_done.T)
        finished += int(o_done.sum())
        successes += int((o_rew == kw.get('max_steps', 300)).sum())
        done_per_env[lo:hi] = o_done.sum(axis=0)
        views = [e.view() for e in ora.envs]
        if frames:
            ish = ora.envs[0].img_shape
            for k, field in (('observation', 'obs'), ('desired_goal', 'desired_img'), ('init_observation', 'init_img')):
                same(k, lo, obs[k][lo:hi].cpu().numpy(), np.stack([np.ctypeslib.as_array(getattr(v, field), shape=ish) for v in views]))
        S = kw['size'][0]
        same('state (agent, hold, achieved, desired, step_num, ep_no)', lo,
             np.stack([st['agent_rc'][lo:hi, 0], st['agent_rc'][lo:hi, 1], st['hold'][lo:hi], st['achieved'][lo:hi], st['desired'][lo:hi],
                       st['step_num'][lo:hi], st['ep_no'][lo:hi]], axis=1).astype(np.int64),
             np.array([(v.agent_r, v.agent_c, v.hold, v.achieved, v.desired, v.step_num, v.ep_no) for v in views], dtype=np.int64))
        same('grid', lo, st['grid'][lo:hi].reshape(n, -1), np.stack([np.ctypeslib.as_array(v.grid, shape=(S * S,)) for v in views]))
        rng = [e.get_rng() for e in ora.envs]
        same('rng position', lo, p2[lo:hi].astype(np.int64), np.array([p for _, p in rng], dtype=np.int64))
        same('rng key', lo, k2[lo:hi], np.stack([k for k, _ in rng]))
        del ora
    return dict(finished=finished, successes=successes, done_per_env=done_per_env)


def assert_counters(env, N, T, res, invalid=0):
    """counters 0..3 of an engine that took T steps of N envs since it was created: env-steps, episodes finished, steps that returned max_steps,
    invalid actions"""
    c = env._counters_raw.cpu().numpy()
    assert (int(c[0]), int(c[1]), int(c[2]), int(c[3])) == (N * T, res['finished'], res['successes'], invalid), c
    return c
