"""Thin host-side adaptors over CraftingWorldVecEnv (no compute here).

* GymnasiumVecAdapter -- the gymnasium (>=0.26 / gymnasium.vector) calling convention:
  reset(seed=...) -> (obs, info), step() -> (obs, reward, terminated, truncated, info).
  terminated = the episode ended by success (reward == MAX_STEPS, ray.py:367), truncated = it ended
  by the step limit only.
* MultiDeviceVecEnv -- one engine + one stream per device driven from ONE process (SURVEY §8e's
  first option; bench.py uses the other, one process per GPU).  Envs are sharded contiguously over
  the devices (sharding.shard_range), no data-path collective; step() enqueues every shard's
  kernels before returning, so the devices run concurrently.
"""
import torch

from .sharding import shard_range
from .vec_env import CraftingWorldVecEnv, as_numpy, desired_bits, reset_mask


class GymnasiumVecAdapter:
    def __init__(self, venv):
        self.venv = venv
        self.num_envs = venv.num_envs
        self.single_observation_space = venv.single_observation_space
        self.single_action_space = venv.single_action_space
        self.observation_space = venv.observation_space
        self.action_space = venv.action_space

    def reset(self, *, seed=None, options=None):
        """options={'reset_mask': m} (gymnasium >= 1.0's vector API): only the envs with m[i] set are reset (venv.reset_envs); not together with
        `seed`, which restarts every env's stream."""
        if options is not None and options.get('reset_mask') is not None:
            if seed is not None:
                raise ValueError("seed= re-seeds every env: it cannot be combined with options['reset_mask']")
            obs = self.venv.reset_envs(mask=options['reset_mask'])
            return obs, {'desired_goal': self.venv.hdr[:, 6:8]}
        if seed is not None:
            self.venv.seed(seed)
        obs = self.venv.reset()
        return obs, {'desired_goal': self.venv.hdr[:, 6:8]}

    def step(self, actions):
        obs, reward, done, info = self.venv.step(actions)
        terminated = done & (reward == self.venv.MAX_STEPS)
        truncated = done & ~terminated
        info = dict(info, _episode=done)                 # gymnasium.vector: which rows of info['episode'] ({'r', 'l'}) hold a finished episode
        if 'terminal_observation' in info:
            info['final_observation'] = info['terminal_observation']
        return obs, reward, terminated, truncated, info

    def close(self):
        self.venv.close()


class MultiDeviceVecEnv:
    """num_envs envs over `devices` (e.g. ['cuda:0', ..., 'cuda:7']); env e's seed is seed+e whatever
    device owns it, so the concatenated result equals a single-device batch of num_envs envs."""

    def __init__(self, num_envs, devices, seed=0, env_menu=None, **kwargs):
        self.devices = [torch.device(d) for d in devices]
        self.num_envs = int(num_envs)
        self.ranges = [shard_range(g, len(self.devices), self.num_envs) for g in range(len(self.devices))]
        self.shards = []
        for (lo, hi), dev in zip(self.ranges, self.devices):
            kw = dict(kwargs)
            if env_menu is not None:
                kw['env_menu'] = env_menu[lo:hi]
            self.shards.append(CraftingWorldVecEnv(hi - lo, device=dev, seed=None if seed is None else seed + lo, **kw))
        self.streams = [torch.cuda.Stream(device=d) for d in self.devices]
        s0 = self.shards[0]
        self.single_observation_space, self.single_action_space = s0.single_observation_space, s0.single_action_space
        self.MAX_STEPS = s0.MAX_STEPS

    def set_rng_states(self, keys, pos):
        for (lo, hi), sh in zip(self.ranges, self.shards):
            sh.set_rng_states(keys[lo:hi], pos[lo:hi])

    def reset(self):
        out = []
        for sh, st in zip(self.shards, self.streams):
            with torch.cuda.stream(st):
                out.append(sh.reset())
        return out

    def reset_envs(self, mask):
        """reset() of the envs with mask[i] set (CraftingWorldVecEnv.reset_envs): the [num_envs] mask is split along self.ranges, each shard's part
        goes to that shard on its own stream; per-shard observation dicts as a list, like reset()."""
        out = []
        for sh, st, m in zip(self.shards, self.streams, self._split_mask(mask, None)):      # (no mask: the first shard's reset_envs raises, as it does alone)
            with torch.cuda.stream(st):
                out.append(sh.reset_envs(mask=m))
        return out

    def _split_mask(self, mask, indices):
        if mask is None and indices is None:
            return [None] * len(self.shards)
        m = reset_mask(self.num_envs, mask=as_numpy(mask), indices=indices)
        return [m[lo:hi] for lo, hi in self.ranges]

    def imagine_obs(self, mask=None, *, indices=None, desired=None, commit=False, one_hot=False):
        """CraftingWorldVecEnv.imagine_obs over the shards: the [num_envs] mask / indices and `desired` ([num_envs] masks or [num_envs, T] rows) are split
        along self.ranges, each part goes to its shard on that shard's stream; -> the shards' result tensors as a list."""
        parts = self._split_mask(mask, indices)
        d = None
        if desired is not None:
            d = desired_bits(self.num_envs, as_numpy(desired), len(self.shards[0].task_list))
        out = []
        for (lo, hi), sh, st, m in zip(self.ranges, self.shards, self.streams, parts):
            with torch.cuda.stream(st):
                out.append(sh.imagine_obs(mask=m, desired=None if d is None else d[lo:hi], commit=commit, one_hot=one_hot))
        return out

    def sample_states(self, mask=None, *, indices=None, pooled=False):
        """CraftingWorldVecEnv.sample_states over the shards, the selection split as in reset_envs; -> the shards' [n, 9] tensors as a list."""
        out = []
        for sh, st, m in zip(self.shards, self.streams, self._split_mask(mask, indices)):
            with torch.cuda.stream(st):
                out.append(sh.sample_states(mask=m, pooled=pooled))
        return out

    def step(self, actions):
        """actions: one tensor per device (already resident there), or a single host/device tensor of
        num_envs actions that is split.  Returns per-device lists [(obs, reward, done, info), ...];
        each shard's results are ordered on that shard's stream (self.streams[g])."""
        if torch.is_tensor(actions) or not isinstance(actions, (list, tuple)):
            actions = torch.as_tensor(actions)
            actions = [actions[lo:hi] for lo, hi in self.ranges]
        out = []
        for sh, st, a in zip(self.shards, self.streams, actions):
            with torch.cuda.stream(st):
                out.append(sh.step(a.to(sh.device, non_blocking=True)))
        return out

    def synchronize(self):
        for st in self.streams:
            st.synchronize()

    def close(self):
        for sh in self.shards:
            sh.close()
