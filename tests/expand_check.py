"""What "an expand call did exactly what it should" means for cw_expand: records_check.check_records_call with a row per (action, state) and
oracle_successors() as what to expect -- the six successors of dense states, each one step of records_check.oracle_simulate.  Pure CPU: numpy arrays in, no
GPU.  A plain module, not a fixture; tests/test_expand_logic.py tests the comparison itself."""
import numpy as np

from records_check import DENSE, check_records_call, oracle_simulate, rows

FIELDS = ('reward', 'done', 'changed', 'achieved_mask', 'hdr', 'slot_pos')
LAYOUT = {f: (6,) for f in FIELDS}


def oracle_successors(states, init_grids, oracle_kw):
    """The six successors of each of M dense states (records_check.decode()'s fields; init_grids uint8 [M, S, S]: the start state of the episode the state
    belongs to): action a is oracle_simulate of the one-step plan a, stepped on whatever ends -> dict of arrays [6, M, ...]: reward, done, changed (the
    oracle's state before and after differs in grid, agent or hold), grid, agent, hold, achieved, desired, step_num and flags -- bit 0 cleared, bit 1
    kept, the count in bits 2-15 one up (saturating) where the oracle's reward is max_steps.  The reward rule is each state's own (flags bit 1);
    oracle_kw: size and max_steps (reward_style in it is ignored)."""
    M = len(states['hold'])
    steps = [oracle_simulate(states, init_grids, np.full((1, M), a), False, oracle_kw) for a in range(6)]
    out = {k: np.stack([s[k] for s in steps]) for k in DENSE}
    out['reward'], out['done'] = np.stack([s['rewards'][0] for s in steps]), np.stack([s['dones'][0] for s in steps])
    out['changed'] = ((out['agent'] != np.asarray(states['agent'])[None]).any(axis=-1) | (out['hold'] != np.asarray(states['hold'])[None])
                      | (out['grid'] != np.asarray(states['grid'])[None]).any(axis=(-1, -2)))
    return out


def check_expand(before, after, inputs, env_of, outputs, sentinel, *, oracle_kw, successors=None):
    """Pure CPU.  cw_expand ran between the snapshots `before` and `after` (masked_check.take()); inputs, env_of, outputs ({field of FIELDS: [6, M, ...]}),
    sentinel and what is compared: records_check.check_records_call.  Row (a, j) of a state that takes part equals the oracle's successor of action a
    from input state j with the start state of its env.
    successors: (dense states, oracle_successors of them) a test has computed already from the oracle's OWN values for the states that take part, in
    order: the records the call read must then decode to exactly these states, and the oracle is not run again.
    -> (states that took part, states skipped)."""
    def expect(states, env, part):
        return successors or (None, oracle_successors(rows(states, part), before['state_init_grid'][env[part]], oracle_kw))
    return check_records_call(before, after, inputs, env_of, outputs, sentinel, name='cw_expand', layout=LAYOUT, expect=expect)
