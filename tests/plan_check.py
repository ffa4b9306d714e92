"""What "a plan call did exactly what it should" means for cw_plan: records_check.check_records_call with a row per (first action, state) and oracle_plan()
as what to expect.  oracle_plan() is nothing but records_check.oracle_simulate(..., stop_at_done=True) over all 6^D action strings of every state, plus
the reduction of craftingworld.h: q[a][j] = the largest return of a string that begins with a, the best plan = the lexicographically smallest string that
reaches it, which is in canonical form (zeros behind its end).  recipe() is the batch of states the tests share, built from the oracle alone, and
coverage() counts what it exercises.  Pure CPU: numpy arrays in, no GPU.  A plain module, not a fixture; tests/test_plan_logic.py tests the comparison
itself."""
import functools

import numpy as np

from records_check import DENSE, check_records_call, oracle_simulate, rows
from simulate_check import RECIPE_KW

FIELDS = ('q', 'length', 'done', 'achieved_mask', 'hdr', 'slot_pos', 'plan')
MAX_DEPTH = 8


def strings(depth):
    """all 6^D action strings in lexicographic order -> int64 [D, 6^D]: column s is string s, its first action the most significant digit"""
    s = np.arange(6 ** depth, dtype=np.int64)
    return np.stack([(s // 6 ** (depth - 1 - t)) % 6 for t in range(depth)])


def oracle_plan(states, init_grids, depth, oracle_kw):
    """M dense states (records_check.decode()'s fields; init_grids uint8 [M, S, S]) -> dict of arrays [6, M, ...]: q, length, done, n_success (1: the best
    plan ends by success), ties (how many distinct TAKEN prefixes reach q: 2 or more = the tie rule decided), plan [6, D, M] and the dense final state of
    the best plan (grid, agent, hold, achieved, desired, step_num, flags).  Every one of the 6^D strings of every state goes through oracle_simulate with
    stop_at_done=True; numpy's argmax returns the FIRST maximum, which in lexicographic order is the smallest maximiser."""
    if not 1 <= depth <= MAX_DEPTH:
        raise ValueError('depth = %d' % depth)
    M = len(states['hold'])
    n, digits = 6 ** depth, strings(depth)
    acts = np.repeat(digits, M, axis=1)                                        # column s * M + j: string s of state j
    tiled = {k: np.tile(np.asarray(states[k]), (n,) + (1,) * (np.asarray(states[k]).ndim - 1)) for k in DENSE}
    r = oracle_simulate(tiled, np.tile(np.asarray(init_grids), (n, 1, 1)), acts, True, oracle_kw)
    ret = r['ret'].reshape(6, n // 6, M)
    q = ret.max(axis=1)
    first = ret.argmax(axis=1) + (np.arange(6) * (n // 6))[:, None]            # [6, M]: the string
    flat = first * M + np.arange(M)[None, :]
    out = dict(q=q, length=r['length'][flat], done=r['done'][flat], n_success=r['n_success'][flat], plan=np.stack([digits[t][first] for t in range(depth)], axis=1))
    behind = np.arange(depth)[None, :, None] >= out['length'][:, None, :]
    assert (out['plan'][behind] == 0).all() and (out['plan'][:, 0] == np.arange(6)[:, None]).all()      # canonical by construction
    tail = 6 ** (depth - r['length'].reshape(6, n // 6, M))                    # a string is the canonical form of its taken prefix iff its tail is zeros
    canon = (np.arange(n).reshape(6, n // 6, 1) % tail) == 0
    out['ties'] = ((ret == q[:, None, :]) & canon).sum(axis=1)
    for k in DENSE:
        out[k] = r[k][flat]
    return out


def layout(depth):
    """{field: the shape in front of the M states}: a row per (first action, state), plan a row per (first action, step, state)"""
    return {f: (6, depth) if f == 'plan' else (6,) for f in FIELDS}


def check_plan(before, after, inputs, env_of, depth, outputs, sentinel, *, oracle_kw, expected=None):
    """Pure CPU.  cw_plan ran between the snapshots `before` and `after` (masked_check.take()); inputs, env_of, outputs ({field of FIELDS: [6, M, ...],
    plan [6, D, M]}), sentinel and what is compared: records_check.check_records_call.  Row (a, j) of a state that takes part, its plan rows included,
    equals oracle_plan of input state j with the start state of its env.
    expected: (dense states, oracle_plan of them) a test has computed already for the states that take part, in order: the records the call read must then
    decode to exactly these states, and the oracle is not run again.  -> (states that took part, states skipped)."""
    def expect(states, env, part):
        return expected or (None, oracle_plan(rows(states, part), before['state_init_grid'][env[part]], depth, oracle_kw))
    return check_records_call(before, after, inputs, env_of, outputs, sentinel, name='cw_plan', layout=layout(depth), expect=expect)


# ------------------------------------------------------------------------------------------------------------------------------ the shared batch of states
RECIPE_N = 600                                  # two full workgroups and a 24-lane tail wave
RECIPE_PART = {1: 600, 2: 600, 3: 600, 4: 100, 5: 24}      # how many of the 600 take part at depth D: the oracle steps 6^D strings of each
RECIPE_SEED = 900


def recipe_env_of(depth):
    """env_of of the recipe at depth D: state j is env j's, RECIPE_PART[D] of them evenly spread take part, the rest hold -1"""
    e = np.full(RECIPE_N, -1, np.int64)
    pick = (np.arange(RECIPE_PART[depth]) * RECIPE_N) // RECIPE_PART[depth]
    e[pick] = pick
    return e


def far_goals(states, init_grids, steps, oracle_kw):
    """for each of M dense states the smallest achieved mask the oracle reaches with some string of steps[j] actions and with NO shorter one (nor holds
    already) -> int64 [M], -1 where there is none: a goal steps[j] steps away, found by the oracle's own enumeration"""
    M = len(states['hold'])
    seen = [{int(states['achieved'][j])} for j in range(M)]
    goal = np.full(M, -1, np.int64)
    for d in range(1, int(np.max(steps)) + 1):
        rows = np.flatnonzero(np.asarray(steps) >= d)
        n = 6 ** d
        tiled = {k: np.tile(np.asarray(states[k])[rows], (n,) + (1,) * (np.asarray(states[k]).ndim - 1)) for k in DENSE}
        tiled['desired'] = np.full(n * len(rows), 0xFFFF, np.int64)                # (no goal: nothing pays)
        ach = oracle_simulate(tiled, np.tile(np.asarray(init_grids)[rows], (n, 1, 1)), np.repeat(strings(d), len(rows), axis=1), False,
                              oracle_kw)['achieved'].reshape(n, len(rows))
        for c, j in enumerate(rows):
            new = set(ach[:, c].tolist()) - seen[j]
            if steps[j] == d and new:
                goal[j] = min(new)
            seen[j] |= new
    return goal


@functools.lru_cache(maxsize=None)
def recipe(depth, style=None):
    """600 states on a 5 x 5 grid, max_steps 17: oracle env j seeded RandomState(900 + j), after reset() and j % 6 steps of a random walk (things held,
    eaten and built).  Those that take part at depth D (recipe_env_of) are dealt into four classes by their rank i.  i % 4 == 0: `desired` := the
    achieved mask the oracle reaches after 1 + (i // 4) % D more steps of the walk, as test_simulate._near_goals builds goals that get satisfied (most
    of them within two steps).  1: `desired` := a mask the oracle reaches after D - (i // 4) % 2 steps and not sooner (far_goals), so that best plans of
    the full length exist -- from depth 4 on class 0 is dealt these too, at depth 5 (24 states) class 3 as well; without such a mask the state stays as it is.  2: step_num := max_steps - 1 -
    (i // 4) % D, the time-out inside the horizon.  3: as it is -- its goal is out of reach, no plan ends.
    -> (dense states [600], init grids [600, 5, 5], env_of [600]); flags: the reward rule `style`, a step taken."""
    from oracle import OracleEnv
    env_of = recipe_env_of(depth)
    rank = {int(j): i for i, j in enumerate(np.flatnonzero(env_of >= 0))}
    max_steps = RECIPE_KW['max_steps']
    st, far = [], {}
    for j in range(RECIPE_N):
        s0 = np.random.RandomState(RECIPE_SEED + j).get_state()
        o = OracleEnv(rng_state=(s0[1].astype(np.uint32), int(s0[2])), reward_style=style, **RECIPE_KW)
        o.reset()
        walk = np.random.RandomState(7000 + j).randint(0, 6, 6 + MAX_DEPTH)
        for a in walk[:j % 6]:
            o.step(int(a))
        s = o.state()
        i = rank.get(j)
        if i is not None and (i % 4 == 1 or i % 4 == 0 and depth >= 4 or i % 4 == 3 and depth >= 5):
            far[j] = depth - (i // 4) % 2
        elif i is not None and i % 4 == 0:
            for a in walk[6:6 + 1 + (i // 4) % depth]:
                o.step(int(a))
            s['desired'] = o.view().achieved
        elif i is not None and i % 4 == 2:
            s['step_num'] = max_steps - 1 - (i // 4) % depth
        st.append(s)
    dense = dict(grid=np.stack([s['grid'] for s in st]), agent=np.array([s['agent'] for s in st], np.int64), hold=np.array([s['hold'] for s in st], np.int64),
                 achieved=np.array([s['achieved'] for s in st], np.int64), desired=np.array([s['desired'] for s in st], np.int64),
                 step_num=np.array([s['step_num'] for s in st], np.int64), flags=np.full(RECIPE_N, 2 if style else 0, np.int64))
    init_grids = np.stack([s['init_grid'] for s in st])
    rows = np.array(sorted(far), np.int64)
    steps = np.array([max(far[j], 1) for j in rows], np.int64)
    goal = far_goals({k: v[rows] for k, v in dense.items()}, init_grids[rows], steps, RECIPE_KW)
    dense['desired'][rows] = np.where(goal >= 0, goal, dense['desired'][rows])
    return dense, init_grids, env_of


@functools.lru_cache(maxsize=None)
def recipe_plans(depth, style=None):
    """(the dense states that take part, oracle_plan of them): computed once, shared by every test of the recipe and left unchanged"""
    dense, init_grids, env_of = recipe(depth, style)
    part = np.flatnonzero(env_of >= 0)
    sub = {k: v[part] for k, v in dense.items()}
    return sub, oracle_plan(sub, init_grids[part], depth, RECIPE_KW)


def coverage(want, depth):
    """what a batch of states exercises, counted over its (first action, state) pairs from oracle_plan alone -> dict: success[L] (the best plan ends by
    success at length L, L = 1 .. D), timeout (it ends inside the horizon without success), never (no plan ends: q = -D), ties (two or more taken
    prefixes reach q), pickup / drop (a best plan that ends by success holds a pick-up / a drop among the steps it takes)"""
    ok = want['done'] & (want['n_success'] > 0)
    taken = np.arange(depth)[None, :, None] < want['length'][:, None, :]
    holds = lambda a: ok & ((want['plan'] == a) & taken).any(axis=1)  # noqa: E731
    return dict(success={L: int((ok & (want['length'] == L)).sum()) for L in range(1, depth + 1)}, timeout=int((want['done'] & ~ok).sum()),
                never=int((~want['done'] & (want['q'] == -depth)).sum()), ties=int((want['ties'] >= 2).sum()), pickup=int(holds(4).sum()), drop=int(holds(5).sum()))


COVERAGE_MIN = 20


def assert_recipe_coverage(covs):
    """covs: {D: coverage of the recipe at depth D} for D = 1 .. 5 under ONE reward rule.  Summed over the depths, at least COVERAGE_MIN pairs each: a best
    plan that succeeds at every length 1 .. 5, one that ends by time-out, a state no plan ends, a tie resolved, a pick-up and a drop inside a best plan"""
    assert sorted(covs) == [1, 2, 3, 4, 5], sorted(covs)
    for L in range(1, 6):
        assert sum(c['success'].get(L, 0) for c in covs.values()) >= COVERAGE_MIN, (L, covs)
    for k in ('timeout', 'never', 'ties', 'pickup', 'drop'):
        assert sum(c[k] for c in covs.values()) >= COVERAGE_MIN, (k, covs)
