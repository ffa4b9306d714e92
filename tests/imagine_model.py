"""imagine_obs() / sample_state() / generate_fixed_initial_state() of the reference (ray.py:220-299, 599-644) restated in numpy on the
(S,S) cell-code grids the tests work with -- TEST INFRASTRUCTURE ONLY: the comparator of the GPU tests (tests/test_imagine.py) and the source of the two
entry points the fake engine gains (tests/fake_engine_imagine.py).  tests/test_imagine_model.py licenses it: every tests/golden/imagine_*.npz fixture,
captured from the reference itself (tools/gen_golden.py, kind 'imagine'), is replayed through it exactly.

Also here: the op script those fixtures hold and its runner, shared by the generator (run on the reference's classes) and the replaying tests (run on
ModelEnv below, and on this package's N=1 classes over the fake and the HIP engine).
"""
import ctypes as C
import glob
import json
import os
import zlib

import numpy as np

STICKS, AXE, HAMMER, ROCK, TREE, BREAD, HOUSE, WHEAT = range(1, 9)
T_MAKEBREAD, T_EATBREAD, T_BUILDHOUSE, T_CHOPTREE, T_CHOPROCK, T_GOTOHOUSE, T_MOVEAXE, T_MOVEHAMMER, T_MOVESTICKS = range(9)
ALL_TASKS = (1 << 9) - 1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------------------------------------ the model
def imagine(init_codes, init_agent, cur_agent, desired, rs, gotohouse_ignores_position=False, movesticks_ignores_agent=False):
    """ray.py:220-299 on cell codes.  init_codes (S,S): the episode's start state (INIT_OBS_VECTOR: one of each of the eight objects -- a bread and a house among them, so every
    branch finds its object -- and nothing held), init_agent its
    agent cell (r, c), cur_agent the env's agent_pos at the call, desired the task bits, rs the numpy RandomState drawn from (same calls, same order).
    -> (goal codes (S,S) uint8, goal agent (r, c)).  np.where walks row-major, as the reference's does.
    gotohouse_ignores_position=True is a deliberately WRONG model (the agent always lands on the house), movesticks_ignores_agent=True another (the sticks
    may land on the agent's cell, as the axe and the hammer may): the tests show that the fixtures catch them."""
    g = np.array(init_codes, dtype=np.uint8)
    agent = (int(init_agent[0]), int(init_agent[1]))
    want = lambda t: (int(desired) >> t) & 1  # noqa: E731
    if want(T_MAKEBREAD):                                     # :226-231
        r, c = np.where(g == WHEAT)
        g[r[0], c[0]] = BREAD
    if want(T_EATBREAD):                                      # :232-237
        r, c = np.where(g == BREAD)
        k = rs.randint(len(r))
        g[r[k], c[k]] = 0
    if want(T_CHOPTREE):                                      # :238-243
        r, c = np.where(g == TREE)
        g[r[0], c[0]] = STICKS
    if want(T_MOVESTICKS):                                    # :244-257 (no object, no agent: channels :9)
        r, c = np.where(g == STICKS)
        k = rs.randint(len(r))
        free = g == 0
        if not movesticks_ignores_agent:
            free[agent] = False
        fr, fc = np.where(free)
        j = rs.randint(len(fr))
        g[r[k], c[k]] = 0
        g[fr[j], fc[j]] = STICKS
    if want(T_BUILDHOUSE):                                    # :258-264
        r, c = np.where(g == STICKS)
        k = rs.randint(len(r))
        g[r[k], c[k]] = HOUSE
    if want(T_CHOPROCK):                                      # :265-268
        r, c = np.where(g == ROCK)
        g[r[0], c[0]] = 0
    if want(T_GOTOHOUSE):                                     # :269-276: channels 8: of the CURRENT cell of the START state move to the house
        r, c = np.where(g == HOUSE)
        k = rs.randint(len(r))
        if gotohouse_ignores_position or (int(cur_agent[0]), int(cur_agent[1])) == agent:
            agent = (int(r[k]), int(c[k]))
    for t, code in ((T_MOVEAXE, AXE), (T_MOVEHAMMER, HAMMER)):   # :277-297 (the agent's cell is allowed: channels :8)
        if want(t):
            r, c = np.where(g == code)
            fr, fc = np.where(g == 0)
            j = rs.randint(len(fr))
            g[r[0], c[0]] = 0
            g[fr[j], fc[j]] = code
    return g, agent


def sample_state(size, rs):
    """ray.py:599-628 -> the nine cells (row * S + col) of objects 0..7 and of the agent: row v of the diagonal block ends where perm holds v"""
    perm = np.arange(size * size)
    rs.shuffle(perm)
    return np.array([int(np.flatnonzero(perm == v)[0]) for v in range(9)], dtype=np.uint16)


def generate_fixed_initial_state(pool, rs):
    """ray.py:630-644: pool uint16 [K, 9] (fixed_state_list as cells) -> one row; randint(0) raises ValueError before any draw"""
    return np.array(pool[rs.randint(len(pool))], dtype=np.uint16)


def codes_of_cells(size, cells):
    g = np.zeros((size, size), np.uint8)
    for k in range(8):
        g[int(cells[k]) // size, int(cells[k]) % size] = k + 1
    return g, (int(cells[8]) // size, int(cells[8]) % size)


def one_hot(codes, agent):
    g = np.asarray(codes)
    oh = np.zeros(g.shape + (12,), dtype=np.uint8)
    r, c = np.nonzero(g)
    oh[r, c, g[r, c] - 1] = 1
    oh[agent[0], agent[1], 8] = 1
    return oh


def render(codes, agent, alt=False):
    """the goal state's frame through the oracle's rasterisers (cwo_render / cwo_render_alt); nothing is held in a goal state"""
    from oracle.oracle import _lib
    lib, u8p = _lib(), C.POINTER(C.c_uint8)
    g = np.ascontiguousarray(codes, dtype=np.uint8)
    s = g.shape[0]
    out = np.empty((3 * s + 3, 3 * s, 3) if alt else (4 * s, 4 * s, 3), dtype=np.uint8)
    fn = lib.cwo_render_alt if alt else lib.cwo_render
    fn.argtypes = [C.c_int32, u8p, C.c_int32, C.c_int32, C.c_int32, u8p]
    fn.restype = None
    fn(s, g.ctypes.data_as(u8p), int(agent[0]), int(agent[1]), 0, out.ctypes.data_as(u8p))
    return out


# ------------------------------------------------------------------------------------------------------------------------------ the op script
I_RESET, I_STEP, I_IMAGINE, I_SAMPLE, I_GENFIXED, I_RANDINT, I_ASSIGN, I_FOREIGN_RANDINT = range(8)
COLS = 10
# I_IMAGINE / I_SAMPLE / I_GENFIXED rows: 0 CRC of the return's uint8 view, 1 dtype (itemsize * 4 + 'iub'.index(kind)), 2 shape (16 bits per dimension),
# 3 CRC of the state's codes (goal state / sampled state), 4 its agent cell r * 256 + c, 5 / 6 np_random's pos / CRC of its key afterwards,
# 7 flags, 8 the desired bits imagined (I_IMAGINE), 9 I_IMAGINE: the agent stood on its start cell.   I_GENFIXED with an empty pool: [-1, ., ., ., ., pos, crc]
COL_RET, COL_DTYPE, COL_SHAPE, COL_STATE, COL_AGENT, COL_POS, COL_KEY, COL_FLAGS, COL_DESIRED, COL_HOME = range(10)
F_NEW, F_GOAL_KEPT, F_INIT_KEPT = 1, 2, 4           # the return is a new object; env.desired_goal / INIT_OBS_VECTOR are unchanged by the call
STATE_COLS = (COL_STATE, COL_AGENT)                 # what only a probe into the callee can fill (the Ray classes return pixels)


def _shape_code(a):
    s = tuple(a.shape) + (0, 0, 0)
    return (s[0] << 32) | (s[1] << 16) | s[2]


def _dtype_code(a):
    return a.dtype.itemsize * 4 + 'iub'.index(a.dtype.kind)


def _rng_cols(env):
    st = env.np_random.get_state()
    return int(st[2]), crc(np.asarray(st[1], np.uint32))


def _codes(oh):
    oh = np.asarray(oh)
    codes = (oh[:, :, :8] * np.arange(1, 9)).sum(axis=2).astype(np.uint8)
    r, c = np.where(oh[:, :, 8] == 1)
    return codes, (int(r[0]), int(c[0]))


def script(policy_seed, rounds=5):
    """the op list of one imagine fixture, built from a policy seed (the generator searches seeds until the reference's run meets the conditions the
    fixtures are to cover; the fixture stores the list)"""
    rs = np.random.RandomState(policy_seed)
    S = []
    add = lambda op, arg=0: S.append((op, int(arg)))  # noqa: E731
    add(I_RESET)
    add(I_IMAGINE, -1)                                         # the env's own vector
    add(I_IMAGINE, 0)                                          # nothing desired: the start state, no draw
    add(I_STEP, 1); add(I_IMAGINE, ALL_TASKS)                  # (usually) off the start cell
    add(I_STEP, 3); add(I_IMAGINE, ALL_TASKS)                  # ... and back on it
    for t in range(9):
        add(I_IMAGINE, 1 << t)
    add(I_IMAGINE, (1 << T_BUILDHOUSE) | (1 << T_GOTOHOUSE) | (1 << T_CHOPTREE))   # two houses: the start state's and the one built
    add(I_SAMPLE)
    add(I_GENFIXED)
    add(I_RANDINT, 1000); add(I_IMAGINE, -1)                   # the caller draws between two calls
    for rnd in range(rounds):
        if rnd == 2:
            add(I_ASSIGN, 1000 + policy_seed)                  # the caller's own RandomState becomes the env's generator
        add(I_RESET)
        for _ in range(int(rs.randint(0, 12))):
            add(I_STEP, int(rs.randint(6)))
        add(I_IMAGINE, -1 if rs.randint(3) == 0 else int(rs.randint(512)))
        if rnd >= 2:
            add(I_FOREIGN_RANDINT, 10 ** 6)
        for _ in range(int(rs.randint(0, 4))):
            add(I_STEP, int(rs.randint(4)))
        add(I_IMAGINE, ALL_TASKS)
        add(I_SAMPLE if rs.randint(2) else I_GENFIXED)
        add(I_IMAGINE, int(rs.randint(512)))
    return np.array([s[0] for s in S], np.int8), np.array([s[1] for s in S], np.int64)


def sweep_script(step_actions):
    """the op list of a sweep fixture (tests/golden/sweep_imagine*_alias.npz): every desired mask 0..511 with the agent on its start cell, the steps
    that take it off (the generator searches a seed at which they do, and asserts it), every mask again"""
    S = [(I_RESET, 0)] + [(I_IMAGINE, m) for m in range(ALL_TASKS + 1)] + [(I_STEP, int(a)) for a in step_actions] + \
        [(I_IMAGINE, m) for m in range(ALL_TASKS + 1)]
    return np.array([s[0] for s in S], np.int8), np.array([s[1] for s in S], np.int64)


def run_script(env, ops, args, state_probe=None):
    """-> (rows int64 [n_ops, COLS], states: the (codes, agent) of every I_IMAGINE / I_SAMPLE / I_GENFIXED op that returned, in order -- filled only with a
    state_probe(env, ret) -> one-hot state or None; without one the STATE_COLS stay 0)."""
    rows = np.zeros((len(ops), COLS), dtype=np.int64)
    states, foreign, last_ret = [], None, None
    for i, (op, arg) in enumerate(zip(ops, args)):
        op, arg = int(op), int(arg)
        row = []
        if op == I_RESET:
            env.reset()
            row = [int(sum(int(b) << t for t, b in enumerate(np.asarray(env.desired_goal_vector).reshape(-1))))] + list(_rng_cols(env))
        elif op == I_STEP:
            _, r, d, _ = env.step(arg)
            row = [int(r), int(bool(d)), env.agent_pos.row * 256 + env.agent_pos.col]
        elif op == I_IMAGINE:
            vec = env.desired_goal_vector
            saved = np.array(vec).copy()
            if arg >= 0:                                       # the caller edits the live vector, calls, and puts the episode's own back
                vec[0, :] = [(arg >> t) & 1 for t in range(vec.shape[1])]
            used = int(sum(int(b) << t for t, b in enumerate(np.asarray(vec).reshape(-1))))
            goal_before, init_before = env.desired_goal, env.INIT_OBS_VECTOR
            goal_crc, init_crc = crc(np.asarray(goal_before).astype(np.uint8)), crc(np.asarray(init_before).astype(np.uint8))
            _, init_agent = _codes(init_before)
            home = int((env.agent_pos.row, env.agent_pos.col) == init_agent)
            ret = env.imagine_obs()
            vec[0, :] = saved[0]
            flags = (F_NEW if (ret is not env.desired_goal and ret is not last_ret and ret is not env.INIT_OBS_VECTOR) else 0) | \
                (F_GOAL_KEPT if (env.desired_goal is goal_before and crc(np.asarray(env.desired_goal).astype(np.uint8)) == goal_crc) else 0) | \
                (F_INIT_KEPT if (env.INIT_OBS_VECTOR is init_before and crc(np.asarray(env.INIT_OBS_VECTOR).astype(np.uint8)) == init_crc) else 0)
            last_ret = ret
            assert int(np.max(ret)) <= 255 and int(np.min(ret)) >= 0
            st = state_probe(env, ret) if state_probe else None
            sc, sa = (0, 0)
            if st is not None:
                codes, agent = _codes(st)
                states.append((codes, agent))
                sc, sa = crc(codes), agent[0] * 256 + agent[1]
            row = [crc(np.asarray(ret).astype(np.uint8)), _dtype_code(ret), _shape_code(ret), sc, sa] + list(_rng_cols(env)) + [flags, used, home]
        elif op in (I_SAMPLE, I_GENFIXED):
            try:
                state, pos = env.sample_state() if op == I_SAMPLE else env.generate_fixed_initial_state()
            except (ValueError, AttributeError):       # an empty pool: the reference fails on the missing fixed_state_list attribute, this package on randint(0)
                row = [-1, 0, 0, 0, 0] + list(_rng_cols(env))
            else:
                codes, agent = _codes(state)
                assert (pos.row, pos.col) == agent and state.shape[2] == 12 and int(np.asarray(state)[:, :, 9:].sum()) == 0
                states.append((codes, agent))
                flags = F_NEW if (state is not env.INIT_OBS_VECTOR and state is not env.obs_one_hot) else 0
                row = [crc(np.asarray(state).astype(np.uint8)), _dtype_code(state), _shape_code(state), crc(codes), agent[0] * 256 + agent[1]] + \
                    list(_rng_cols(env)) + [flags]
        elif op == I_RANDINT:
            row = [int(env.np_random.randint(arg))]
        elif op == I_ASSIGN:
            foreign = np.random.RandomState(arg)
            env.np_random = foreign
            row = [int(env.np_random is foreign)]
        elif op == I_FOREIGN_RANDINT:
            row = [int(foreign.randint(arg))]
        else:
            raise ValueError('unknown op %d' % op)
        rows[i, :len(row)] = row
    return rows, states


def fixture_names():
    return sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(GOLDEN, 'imagine_*.npz')))


def sweep_fixture_names():
    return sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(GOLDEN, 'sweep_imagine*_alias.npz')))


def load(name):
    z = np.load(os.path.join(GOLDEN, name + '.npz'))
    d = {k: z[k] for k in z.files}
    meta = json.loads(bytes(d.pop('meta')).decode())
    kw = dict(meta['kwargs'])
    if 'size' in kw:
        kw['size'] = tuple(kw['size'])
    return meta, kw, d


# ------------------------------------------------------------------------------------------------------------------------------ the model as an env
class _Pos:
    def __init__(self, r, c):
        self.row, self.col = int(r), int(c)


class ModelEnv:
    """What run_script needs of a reference env: reset() / step() by the C oracle (itself pinned to the reference by tests/test_oracle_golden.py), the three
    goal-drawing methods by the model above on a numpy RandomState that carries the oracle's stream across each call."""

    def __init__(self, env_name, key, pos, wrong=False, **kw):
        """wrong: False, True / 'gotohouse' or 'movesticks' -- which deliberately wrong variant of imagine() to run"""
        from oracle import OracleEnv
        self._alt, self._onehot = env_name == 'CraftingWorldEnvAltObs', env_name == 'CraftingWorldEnvOneHot'
        kw = dict(kw)
        kw.pop('stacked_obs', None)
        self._ora = OracleEnv(rng_state=(key, pos), alt_obs=self._alt, **kw)
        self._wrong = wrong
        self.size = self._ora.size
        self.np_random = np.random.RandomState()
        self._pull_rng()
        self.desired_goal_vector = np.zeros((1, self._ora.n_task_list), dtype=int)

    def _pull_rng(self):
        k, p = self._ora.get_rng()
        st = self.np_random.get_state()
        self.np_random.set_state(('MT19937', k, p, st[3], st[4]))

    def _push_rng(self):
        st = self.np_random.get_state()
        self._ora.set_rng(np.asarray(st[1], np.uint32), int(st[2]))

    @property
    def agent_pos(self):
        return _Pos(*self._ora.state()['agent'])

    @property
    def obs_one_hot(self):
        return None

    def reset(self):
        self._push_rng()
        self._ora.reset()
        self._pull_rng()
        s = self._ora.state()
        self.desired_goal_vector = np.array([[(s['desired'] >> t) & 1 for t in range(self._ora.n_task_list)]], dtype=int)
        self.INIT_OBS_VECTOR = one_hot(s['init_grid'], s['init_agent'])
        self.desired_goal = one_hot(s['goal_grid'], s['goal_agent']) if self._onehot else s['desired_img']
        self._init = (s['init_grid'], tuple(s['init_agent']))

    def step(self, a):
        o, r, d, info = self._ora.step(a)
        return o, r, d, info

    def imagine_obs(self):
        bits = int(sum(int(b) << t for t, b in enumerate(self.desired_goal_vector[0])))
        codes, agent = imagine(self._init[0], self._init[1], self._ora.state()['agent'], bits, self.np_random,
                               gotohouse_ignores_position=self._wrong in (True, 'gotohouse'), movesticks_ignores_agent=self._wrong == 'movesticks')
        self._push_rng()
        self.last_state = one_hot(codes, agent)
        return self.last_state.astype(np.int64) if self._onehot else render(codes, agent, self._alt).astype(np.int64)

    def _placed(self, cells):
        codes, agent = codes_of_cells(self.size, cells)
        self._push_rng()
        return one_hot(codes, agent).astype(np.int64), _Pos(*agent)

    def sample_state(self):
        return self._placed(sample_state(self.size, self.np_random))

    def generate_fixed_initial_state(self):
        if not self._ora.cfg.fixed_init_state:
            raise ValueError('high <= 0')
        return self._placed(generate_fixed_initial_state(self._ora.fixed_states(), self.np_random))
