"""What "a simulate call did exactly what it should" means for cw_simulate: records_check.check_records_call with a row per state, a trace row per step
and state, and records_check.oracle_simulate as what to expect.  recipe() is the batch of states and plans the tests share, built from the oracle alone,
and coverage() counts what it exercises.  Pure CPU: numpy arrays in, no GPU.  A plain module, not a fixture; tests/test_simulate_logic.py tests the
comparison itself."""
import functools

import numpy as np

from records_check import check_records_call, oracle_simulate, rows

FIELDS = ('ret', 'length', 'done', 'achieved_mask', 'hdr', 'slot_pos', 'rewards', 'dones')
PER_STATE, TRACES = FIELDS[:6], FIELDS[6:]


def layout(T):
    """{field: the shape in front of the M states}: a row per state, the traces a row per step and state"""
    return {f: (T,) if f in TRACES else () for f in FIELDS}


def check_simulate(before, after, inputs, env_of, actions, stop_at_done, outputs, sentinel, *, oracle_kw, expected=None):
    """Pure CPU.  cw_simulate ran between the snapshots `before` and `after` (masked_check.take()); inputs (None: the engine's own states, broadcast:
    state j is before['hdr'][j % N], M = the actions' columns), env_of, outputs ({field of FIELDS: [M, ...] or [T, M]}), sentinel and what is compared:
    records_check.check_records_call.  actions [T, M] (any trailing shape of M columns).  Every row of a state that takes part, trace rows included,
    equals oracle_simulate of input state j with the start state of its env.
    expected: (dense states, oracle_simulate of them) a test has computed already for the states that take part, in order: the records the call read must
    then decode to exactly these states, and the oracle is not run again.  -> (states that took part, states skipped)."""
    acts = np.asarray(actions)
    if acts.ndim < 2:
        raise ValueError('actions must be [T, M], got %s' % (acts.shape,))
    acts = acts.reshape(acts.shape[0], -1)

    def expect(states, env, part):
        return expected or (None, oracle_simulate(rows(states, part), before['state_init_grid'][env[part]], acts[:, part], stop_at_done, oracle_kw))
    return check_records_call(before, after, inputs, env_of, outputs, sentinel, name='cw_simulate', layout=layout(acts.shape[0]), expect=expect,
                              M=acts.shape[1])


# ------------------------------------------------------------------------------------------------------------------------------ the shared batch of plans
RECIPE_N, RECIPE_KW = 600, dict(size=(5, 5), max_steps=17)


@functools.lru_cache(maxsize=None)
def recipe(T, style=None):
    """600 states on a 5 x 5 grid, max_steps 17: oracle envs seeded RandomState(900 + j) after reset(); actions RandomState(7).randint(0, 6, (T, 600)); for
    even j `desired` is replaced by the achieved mask the oracle itself reaches after 2 + (j // 2) % 9 steps of its own column (without the relabel 2-3
    of 600 ever succeed).  -> (dense states, init grids [600, 5, 5], actions int64 [T, 600]); flags: the reward rule `style`, no step taken yet."""
    from oracle import OracleEnv
    acts = np.random.RandomState(7).randint(0, 6, (T, RECIPE_N))
    st = []
    for j in range(RECIPE_N):
        s0 = np.random.RandomState(900 + j).get_state()
        o = OracleEnv(rng_state=(s0[1].astype(np.uint32), int(s0[2])), reward_style=style, **RECIPE_KW)
        o.reset()
        s = o.state()
        if j % 2 == 0:
            for t in range(2 + (j // 2) % 9):
                o.step(int(acts[t, j]))
            s['desired'] = o.view().achieved
        st.append(s)
    dense = dict(grid=np.stack([s['grid'] for s in st]), agent=np.array([s['agent'] for s in st], np.int64), hold=np.array([s['hold'] for s in st], np.int64),
                 achieved=np.array([s['achieved'] for s in st], np.int64), desired=np.array([s['desired'] for s in st], np.int64),
                 step_num=np.array([s['step_num'] for s in st], np.int64), flags=np.full(RECIPE_N, 1 | (2 if style else 0), np.int64))
    return dense, np.stack([s['init_grid'] for s in st]), acts


def coverage(stepped_on, max_steps):
    """what a batch of plans exercises, counted from oracle_simulate(..., stop_at_done=False) alone -> dict: never (no step done), success_first /
    timeout_first (the first done step paid max_steps / did not), success_steps (the distinct step indices that paid), paid_after_done (success rewards
    behind a state's first done step)"""
    rew, T = stepped_on['rewards'], stepped_on['rewards'].shape[0]
    first = stepped_on['length'] - 1
    cols = np.arange(rew.shape[1])
    paid_first = stepped_on['done'] & (rew[np.minimum(first, T - 1), cols] == max_steps)
    behind = np.arange(T)[:, None] > first[None, :]
    return dict(never=int((~stepped_on['done']).sum()), success_first=int(paid_first.sum()), timeout_first=int((stepped_on['done'] & ~paid_first).sum()),
                success_steps=sorted(set(np.nonzero(rew == max_steps)[0].tolist())),
                paid_after_done=int(((rew == max_steps) & behind & stepped_on['done'][None, :]).sum()))


def assert_recipe_coverage(cov12, cov24):
    """the conditions every test of the recipe asserts before anything is compared: each of the three classes 200 times across the two horizons, successes
    at 8 distinct step indices, 500 success rewards behind a first done"""
    assert cov12['never'] >= 200 and cov12['success_first'] >= 200 and cov24['success_first'] >= 200 and cov24['timeout_first'] >= 200, (cov12, cov24)
    assert len(cov12['success_steps']) >= 8 and cov12['paid_after_done'] >= 500, cov12
