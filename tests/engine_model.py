"""The batch engine's state-changing calls on the CPU -- TEST INFRASTRUCTURE ONLY.  EngineModel is an OracleBatch (the reference's dynamics, pinned by
tests/test_oracle_golden.py) plus the calls CraftingWorldVecEnv adds to it: reset_envs, imagine_obs(commit=), sample_states, the snapshot bank,
set_state, set_rng_states and checkpoints, so that ANY sequence of them can be checked after every call (tests/test_call_sequences.py).  It states no
rule of its own: the goal draws are masked_check.model_imagine / model_sample (imagine_model.py, pinned to the reference by its fixtures) on each env's
own stream, the bank's row rules are snapshot_check.sources, and what a row holds, with and without the stream, is the oracle's cwo_copy; a state is
injected with cwo_set_full.  expected() is the oracle's side of oracle_replay.snapshot(): same_states() compares an engine with `model.ora` directly.
as_take() dresses the model as masked_check.take() for the per-call checkers.  A plain module, not a fixture; tests/test_engine_model_logic.py tests
it, and shows with deliberately wrong variants (`defect`) that the comparison catches each at its op."""
import numpy as np

from masked_check import model_imagine, model_sample
from oracle_replay import FRAMES, STATE, oracle_arrays
from snapshot_check import SKIPPED, sources

DEFECTS = ('load_takes_stream', 'reset_envs_keeps_stream', 'commit_keeps_goal_grid', 'set_state_ignores_step_num', 'skipped_not_counted')
COUNTERS = (0, 1, 2, 3, SKIPPED)                     # env-steps, finished, successes, invalid actions, snapshot rows skipped: the rest depends on scheduling
_ORACLE_NAME = dict(agent_rc='agent', init_agent_rc='init_agent', goal_agent_rc='goal_agent')


def _rows(mask, n):
    """the envs a mask selects (None: every env; any non-zero byte selects)"""
    if mask is None:
        return np.arange(n)
    m = np.asarray(mask).reshape(-1)
    if len(m) != n:
        raise ValueError('%d mask bytes for %d envs' % (len(m), n))
    return np.flatnonzero(m)


class EngineModel:
    def __init__(self, N, keys, pos, auto_reset, kw, per_env_kwargs=None, defect=None):
        """N envs from the RNG states (keys, pos), `kw` the configuration as the oracle takes it (oracle_replay.oracle_kw), per_env_kwargs [N] what env i
        adds to it (its task menu).  defect: None, or one of DEFECTS -- a deliberately WRONG model."""
        from oracle import OracleBatch
        if defect is not None and defect not in DEFECTS:
            raise ValueError('unknown defect %r' % (defect,))
        self.N, self.auto_reset, self.defect = int(N), bool(auto_reset), defect
        self.max_steps, self.alt, self.K = kw.get('max_steps', 300), bool(kw.get('alt_obs')), kw.get('fixed_init_state', 0)
        self.ora = OracleBatch(self.N, rng_states=[(keys[i], int(pos[i])) for i in range(self.N)], per_env_kwargs=per_env_kwargs, **kw)
        self.counters = np.zeros(8, np.int64)
        self.reward, self.done = np.zeros(self.N, np.int32), np.zeros(self.N, bool)
        self.bank, self.capacity = {}, 0
        self._menus = []                             # menu ids in order of first appearance (env_menu = arange(N) % n_menus gives the engine's)
        for e in self.ora.envs:
            if e.menu() not in self._menus:
                self._menus.append(e.menu())

    # ---------------------------------------------------------------------------------------------------------------------- episodes
    def reset(self):
        self.ora.reset()

    def _count(self, rew, done):
        self.counters[0] += rew.size
        self.counters[1] += int(np.sum(done))
        self.counters[2] += int(np.sum(rew == self.max_steps))
        self.reward, self.done = np.array(rew[-1] if rew.ndim == 2 else rew, np.int32), np.array(done[-1] if done.ndim == 2 else done, bool)

    def step(self, actions):
        """one step -> (reward int32 [N], done bool [N]); on the auto-reset engine the finished envs are reset"""
        rew, done = self.ora.step(np.asarray(actions).reshape(-1), auto_reset=self.auto_reset)
        self._count(rew, done)
        return rew, done

    def steps(self, actions):
        """T steps, every finished env reset after its step -- the auto-reset engine's step(), step_many(), replayed graph and rollout(), and the manual
        engine's step() + reset_envs(env.done) -> (rewards int32 [T, N], dones bool [T, N])"""
        a = np.asarray(actions)
        total, rew, done = self.ora.rollout(a.astype(np.int8), nthreads=1, record=True)
        assert total == a.size
        self._count(rew, done.astype(bool))
        return rew, done.astype(bool)

    def reset_envs(self, mask):
        for i in _rows(mask, self.N):
            e = self.ora.envs[i]
            rng = e.get_rng()
            e._lib.cwo_reset(e._h)
            if self.defect == 'reset_envs_keeps_stream':
                e.set_rng(*rng)

    # ---------------------------------------------------------------------------------------------------------------------- goal draws
    def _streams(self):
        a = oracle_arrays(self.ora.envs, ['rng_key'])
        return a, a['rng_key'], a['rng_pos']

    def _push(self, rows, keys, pos):
        for j, i in enumerate(rows):
            self.ora.envs[i].set_rng(keys[j], int(pos[j]))

    def imagine_obs(self, mask=None, desired=None, commit=False):
        """-> (the selected rows, goal grids uint8 [n, S, S], goal agents [n, 2]); each selected env's stream advances by its draws.  desired: [N] task
        bits (None: each env's own); commit: the drawn goal -- and `desired`, when given -- becomes the episode's."""
        rows = _rows(mask, self.N)
        st, keys, pos = self._streams()
        n_bits = self.ora.envs[0].n_task_list
        used = st['desired'] if desired is None else np.asarray(desired).reshape(-1).astype(np.int64) & ((1 << n_bits) - 1)
        g, a, k2, p2 = model_imagine(st, keys, pos, rows, used)
        self._push(rows, k2, p2)
        if commit:
            for j, i in enumerate(rows):
                new = dict(goal_agent=a[j])
                if self.defect != 'commit_keeps_goal_grid':
                    new['goal_grid'] = g[j]
                if desired is not None:
                    new['desired'] = int(used[i])
                self.ora.envs[i].update(**new)
        return rows, g, a

    def sample_states(self, mask=None, pooled=False):
        """-> (the selected rows, cells uint16 [n, 9]): sample_state(), or with pooled generate_fixed_initial_state(), from each selected env's stream"""
        if pooled and not self.K:
            raise ValueError('pooled needs fixed_init_state > 0')
        rows = _rows(mask, self.N)
        _, keys, pos = self._streams()
        pool = np.stack([e.fixed_states() for e in self.ora.envs]) if pooled else None
        cells, k2, p2 = model_sample(self.ora.envs[0].size, keys, pos, rows, pool)
        self._push(rows, k2, p2)
        return rows, cells

    # ---------------------------------------------------------------------------------------------------------------------- the bank
    def snapshot_reserve(self, capacity):
        self.bank, self.capacity = {}, int(capacity)

    def _skip(self, n):
        if self.defect != 'skipped_not_counted':
            self.counters[SKIPPED] += n

    def snapshot_save(self, rows):
        """env i into row rows[i] (negative: no part; at or above the capacity: skipped and counted)"""
        rows = np.asarray(rows).reshape(-1)
        for r, i in sources(rows, self.capacity).items():
            self.bank[r] = self.ora.envs[i].clone()
        self._skip(int((rows >= self.capacity).sum()))

    def snapshot_load(self, rows, with_stream=True):
        """env i from row rows[i]; a row outside the bank and a row never saved are skipped and counted -> the envs that were loaded"""
        rows = np.asarray(rows).reshape(-1)
        good = [i for i in range(self.N) if 0 <= rows[i] < self.capacity and int(rows[i]) in self.bank]
        for i in good:
            self.ora.envs[i].copy_from(self.bank[int(rows[i])], with_stream or self.defect == 'load_takes_stream')
        self._skip(int((rows >= 0).sum()) - len(good))
        return np.array(good, dtype=np.int64)

    # ---------------------------------------------------------------------------------------------------------------------- injection
    def set_state(self, **fields):
        """any subset of get_state()'s fields, [N, ...] each"""
        if set(fields) - set(STATE):
            raise ValueError('cannot set %s' % sorted(set(fields) - set(STATE)))
        if self.defect == 'set_state_ignores_step_num':
            fields.pop('step_num', None)
        for i, e in enumerate(self.ora.envs):
            e.update(**{_ORACLE_NAME.get(k, k): np.asarray(v)[i] for k, v in fields.items()})

    def set_rng_states(self, keys, pos):
        for i, e in enumerate(self.ora.envs):
            e.set_rng(keys[i], int(pos[i]))

    def checkpoint(self):
        """everything a checkpoint file holds: every env with its stream, pool and menu, counters 0-3 and the last step's outputs -- not the bank, and not
        the bank's count of skipped rows (counters[6]), which goes on counting across a restore"""
        return [e.clone() for e in self.ora.envs], self.counters.copy(), self.reward.copy(), self.done.copy()

    def restore(self, ckpt):
        envs, counters, reward, done = ckpt
        for e, c in zip(self.ora.envs, envs):
            e.copy_from(c, True)
        self.counters[:4], self.reward, self.done = counters[:4], reward.copy(), done.copy()

    # ---------------------------------------------------------------------------------------------------------------------- what the engine must show
    def expected(self, frames=(), rng=True):
        """the entries oracle_replay.snapshot(env, frames=frames, rng=rng) returns, of the model"""
        out = oracle_arrays(self.ora.envs, list(frames) + (['rng_key', 'rng_pos'] if rng else []))
        out['idx'] = np.arange(self.N)
        return out

    def menu_ids(self):
        return np.array([self._menus.index(e.menu()) for e in self.ora.envs], np.uint8)


def model_for(kind, size, keys, pos, defect=None):
    """the model of the engine `kind` (engines.ENGINES, 'pixels_ray_auto') at size x size, max_steps as engines.K5 -> (model, the engine's own kwargs)"""
    from engines import ENGINES, MENUS, N1, k_of
    from oracle_replay import oracle_kw
    ekw = dict(dict(ENGINES, pixels_ray_auto=dict(obs_mode='pixels', raster='ray'))[kind])
    kw = oracle_kw(dict(k_of(size), fixed_init_state=ekw.get('fixed_init_state', 0)), ekw.get('raster', 'ray'))
    per_env = [MENUS[int(m)] for m in ekw['env_menu']] if 'env_menu' in ekw else None
    return EngineModel(N1, keys, pos, ekw.get('auto_reset', True), kw, per_env, defect), dict(ekw, **k_of(size))


def apply(model, name, args, pending):
    """one op of a sequence_script script on the model -> what the op returned: {'reward', 'done'} [T, N] of 'steps', {'rows', 'goal_grid', 'goal_agent'}
    of an imagine, {'rows', 'cells'} of 'sample', {'good'} of a load, else {}.  pending: the caller's list of checkpoints saved and not yet loaded."""
    from sequence_script import rng_states
    if name == 'steps':
        rew, done = model.steps(args['actions'])
        return dict(reward=rew, done=done)
    if name == 'reset':
        model.reset()
    elif name == 'reset_envs':
        model.reset_envs(args['mask'])
    elif name in ('imagine', 'imagine_commit'):
        rows, g, a = model.imagine_obs(args['mask'], args['desired'], commit=name == 'imagine_commit')
        return dict(rows=rows, goal_grid=g, goal_agent=a)
    elif name == 'sample':
        rows, cells = model.sample_states(args['mask'], args['pooled'])
        return dict(rows=rows, cells=cells)
    elif name == 'save':
        model.snapshot_save(args['rows'])
    elif name in ('load_stream', 'load_episode'):
        return dict(good=model.snapshot_load(args['rows'], with_stream=name == 'load_stream'))
    elif name == 'set_phase':
        model.set_state(step_num=args['phases'])
    elif name == 'set_rng':
        model.set_rng_states(*rng_states(model.N, args['base']))
    elif name == 'ckpt_save':
        pending.append(model.checkpoint())
    elif name == 'ckpt_load':
        model.restore(pending.pop(0))
    else:
        raise ValueError('unknown op %r' % (name,))
    return {}


def compare(snap, counters, model):
    """an engine -- oracle_replay.snapshot() of it and its raw counters -- against the model: everything the snapshot holds through same_states, and
    the COUNTERS"""
    from oracle_replay import same_states
    same_states(snap, model.ora, frames=tuple(k for k in snap if k in FRAMES), rng='rng_key' in snap)
    got, want = [int(counters[k]) for k in COUNTERS], [int(model.counters[k]) for k in COUNTERS]
    assert got == want, 'counters %s (env-steps, finished, successes, invalid, snapshot rows skipped): %s, the model has %s' % (list(COUNTERS), got, want)


def as_take(model, pixels=False):
    """the model as masked_check.take() shows an engine: expected() under take()'s names, plus the entries only an engine has, filled from the model --
    hdr (bytes 0-2 agent and hold, 3 the menu id, 4-5 achieved, 6-7 desired, 8-9 step_num), achieved_mask / desired_mask, reward, done, the counters; the
    slot order and the episode statistics are not modelled and stand as zeros, which every checker then requires to stay"""
    x = model.expected(tuple(FRAMES) if pixels else ())
    N = model.N
    snap = {'state_' + k: x[k] for k in STATE}
    snap['rng_key'], snap['rng_pos'] = x['rng_key'], x['rng_pos']
    hdr = np.zeros((N, 16), np.uint8)
    hdr[:, 0:2], hdr[:, 2], hdr[:, 3] = x['agent_rc'], x['hold'], model.menu_ids()
    for at, k in ((4, 'achieved'), (6, 'desired'), (8, 'step_num')):
        hdr[:, at], hdr[:, at + 1] = x[k] & 0xFF, x[k] >> 8
    snap.update(hdr=hdr, slot_pos=np.zeros((N, 8), np.int16), reward=model.reward.copy(), done=model.done.copy(),
                achieved_mask=x['achieved'].astype(np.uint16), desired_mask=x['desired'].astype(np.uint16),
                episode_length=np.zeros(N, np.int32), episode_return=np.zeros(N, np.int32), counters=model.counters.copy())
    for k in (FRAMES if pixels else ()):
        snap[k] = x[k]
    return snap
