#!/usr/bin/env python3
"""Record what the REFERENCE classes answer on this project's own transition tables (build container only).

tests/state_tables.py builds the tables (local_table: 18 816 states on 5 x 5; wall_table at every wall of 8 x 8: 1 296 states); they are
deterministic, so a fixture stores no grid -- only the CRC32 of each input array, the desired masks and, per (action, state), what
CraftingWorldEnvRay made of the state: achieved mask, agent cell, hold, the code left in the start cell and in the cell the agent ends on, and
per (reward rule, step_num, action, state) reward and done.  walls8_ray_alt adds the CRC32 of both classes' obs_image.astype(uint8) after the step.

Each state is INJECTED into a reference env (obs_one_hot, INIT_OBS_VECTOR, agent_pos, both goal vectors, step_num, obs_image = render(obs_one_hot))
and stepped once; nothing of the reference's text is restated here.  Checked on every row: the one-hot stays valid, no cell changes but the
start cell and the end cell, CraftingWorldEnvAltObs gives the same dynamics, reward and done as CraftingWorldEnvRay.  The files are written with fixed
zip timestamps: two runs give identical bytes.

    python tools/gen_table_golden.py            # both fixtures
    python tools/gen_table_golden.py table5_ray

tests/test_table_golden_logic.py, tests/test_oracle_table.py (CPU) and tests/test_reference_table.py (gpu) read the fixtures; none imports this file.
"""
import io
import json
import os
import sys
import time
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, '..', 'tests'))
from refharness import bits, codes_from_onehot, crc, import_reference, make_ref_env  # noqa: E402
import state_tables as T  # noqa: E402

OUT = os.path.join(HERE, '..', 'tests', 'golden')
CAP = 128 * 1024
RULES = (None, 'subset')                           # reward_style: None is the equal rule, anything else the subset rule (ray.py:71-74)


def one_hot(grid, agent, hold):
    """codes [S, S] (+ agent cell and hold, or None: an init grid) -> the reference's int one-hot state [S, S, 12]"""
    oh = np.zeros(grid.shape + (12,), dtype=int)
    r, c = np.nonzero(grid)
    oh[r, c, grid[r, c] - 1] = 1
    if agent is not None:
        oh[agent[0], agent[1], 8] = 1
        if hold:
            oh[agent[0], agent[1], 8 + hold] = 1
    return oh


def vec(mask):
    return np.array([[(int(mask) >> b) & 1 for b in range(9)]], dtype=int)


class Injected:
    """one reference env per (class, reward rule); put(state) then env.step(a)"""

    def __init__(self, cls, style, S, max_steps):
        self.env = make_ref_env(cls, np.random.RandomState(0), size=(S, S), max_steps=max_steps, reward_style=style)
        self.env.reset()
        self.S = S
        from gym_craftingworld.envs.coordinates import Coord
        self.Coord = Coord

    def put(self, oh, init_oh, agent, achieved, desired, step_num, image):
        e = self.env
        e.obs_one_hot = oh.copy()
        e.INIT_OBS_VECTOR = init_oh                # (never written by step())
        e.agent_pos = self.Coord(int(agent[0]), int(agent[1]), self.S - 1, self.S - 1)
        e.achieved_goal_vector = vec(achieved)
        e.desired_goal_vector = vec(desired)
        e.step_num = int(step_num)
        e.obs_image = image.copy()
        e.observation = {'observation': e.obs_image, 'desired_goal': e.desired_goal, 'achieved_goal': e.obs_image, 'init_observation': e.INIT_OBS}

    def step(self, a):
        _, reward, done, info = self.env.step(a)
        codes, agent, hold = codes_from_onehot(self.env.obs_one_hot)      # (asserts a valid one-hot)
        assert agent == self.env.agent_pos.tuple()
        return int(reward), bool(done), bits(info['achieved_goal']), codes, agent, hold


def run_table(name, classes, frames, log):
    spec = T.TABLE_FIXTURES[name]
    (grid, init, agent, hold, ach), cases = T.fixture_table(name)
    n, S, max_steps, step_nums = len(cases), spec['S'], spec['max_steps'], spec['step_nums']
    envs = {(key, ri): Injected(classes[key], style, S, max_steps) for key in ('ray', 'altobs') for ri, style in enumerate(RULES)}
    ohs = [one_hot(grid[j], agent[j], int(hold[j])) for j in range(n)]
    inits = [one_hot(init[j], None, 0) for j in range(n)]
    imgs = {key: [envs[key, 0].env.render(ohs[j]) for j in range(n)] for key in ('ray', 'altobs')}

    # ---- the desired masks: RandomState(1); for a state drawn with rand() < 0.5 the reference's achieved mask after action i % 6 (0 -> 1), else randint(1, 512)
    rng = np.random.RandomState(1)
    desired = np.zeros(n, np.uint16)
    near = 0
    for i in range(n):
        if rng.rand() < 0.5:
            e = envs['ray', 0]
            e.put(ohs[i], inits[i], agent[i], ach[i], 1, step_nums[0], imgs['ray'][i])
            desired[i] = e.step(i % 6)[2] or 1
            near += 1
        else:
            desired[i] = rng.randint(1, 512)

    cols = dict(achieved=np.zeros((6, n), np.uint16), agent=np.zeros((6, n, 2), np.uint8), hold=np.zeros((6, n), np.uint8), own=np.zeros((6, n), np.uint8),
                new=np.zeros((6, n), np.uint8), reward=np.zeros((2, len(step_nums), 6, n), np.int8), done=np.zeros((2, len(step_nums), 6, n), np.uint8))
    if frames:
        cols['crc_ray'], cols['crc_alt'] = np.zeros((6, n), np.uint32), np.zeros((6, n), np.uint32)
    rows = alt_dynamics_differ = alt_outcome_differ = 0
    over = 0
    t0 = time.time()
    for j in range(n):
        g0 = grid[j]
        for a in range(6):
            first = None
            for ri in range(2):
                for si, sn in enumerate(step_nums):
                    got = {}
                    for key in ('ray', 'altobs'):
                        e = envs[key, ri]
                        e.put(ohs[j], inits[j], agent[j], ach[j], desired[j], sn, imgs[key][j])
                        reward, done, achieved, codes, ag, hd = e.step(a)
                        assert e.env.step_num == sn + 1
                        # no cell changes other than the agent's start cell and the cell it ends on
                        diff = np.argwhere(codes != g0)
                        assert all(tuple(c) in (tuple(agent[j]), ag) for c in diff.tolist()), (name, j, a, diff.tolist())
                        got[key] = (achieved, ag, hd, int(codes[tuple(agent[j])]), int(codes[ag]), reward, done)
                        rows += 1
                        if frames and (ri, si) == (0, 0):
                            img = e.env.obs_image
                            over += int(img.max() > 255)
                            cols['crc_ray' if key == 'ray' else 'crc_alt'][a, j] = crc(img.astype(np.uint8))
                    ray, alt = got['ray'], got['altobs']
                    alt_dynamics_differ += ray[:5] != alt[:5]
                    alt_outcome_differ += ray[5:] != alt[5:]
                    if first is None:
                        first = ray[:5]
                        cols['achieved'][a, j], cols['agent'][a, j], cols['hold'][a, j], cols['own'][a, j], cols['new'][a, j] = ray[:5]
                    assert ray[:5] == first, (name, j, a, 'the dynamics depend on the reward rule or on step_num')
                    assert ray[5] in (-1, max_steps)
                    cols['reward'][ri, si, a, j], cols['done'][ri, si, a, j] = ray[5], ray[6]
    log('%s: %d states (%d goals one step away), %d reference steps (%d per class) in %.0f s' % (name, n, near, rows, rows // 2, time.time() - t0))
    log('%s: CraftingWorldEnvAltObs dynamics %s CraftingWorldEnvRay (%d rows differ), reward / done %s (%d rows differ)' % (
        name, 'EQUAL' if not alt_dynamics_differ else 'DIFFER FROM', alt_dynamics_differ, 'EQUAL' if not alt_outcome_differ else 'DIFFER', alt_outcome_differ))
    if frames:
        log('%s: %d frames hold a value above 255 (stored modulo 256)' % (name, over))
    assert not alt_dynamics_differ and not alt_outcome_differ, 'a finding: store the AltObs rows under their own prefix and say so'
    meta = dict(name=name, table=spec['table'], S=S, max_steps=max_steps, step_nums=step_nums, n=n, env='CraftingWorldEnvRay',
                checked_equal=['CraftingWorldEnvAltObs'], rules=['equal', 'subset'], desired_seed=1, input_crc=T.input_crcs((grid, init, agent, hold, ach)))
    return dict(cols, desired=desired, meta=np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8))


def write_npz(path, arrays):
    """np.savez_compressed with the members in sorted order and a fixed timestamp: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    only = set(sys.argv[1:])
    classes = import_reference()
    os.makedirs(OUT, exist_ok=True)
    for name in T.TABLE_FIXTURES:
        if only and name not in only:
            continue
        out = run_table(name, classes, name == 'walls8_ray_alt', print)
        path = os.path.join(OUT, name + '.npz')
        write_npz(path, out)
        size = os.path.getsize(path)
        print('%s: %d rows of dynamics, %d of reward / done, %.1f KB' % (name, 6 * len(out['desired']), out['reward'].size, size / 1024))
        assert size < CAP, 'split by action, do not thin the table'
        T.load_table_fixture(name, path)


if __name__ == '__main__':
    main()
