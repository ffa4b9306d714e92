"""The conditions the call-sequence scripts (tests/sequence_script.py) have to meet for tests/test_call_sequences.py to mean what it says, checked from the
CPU model alone (tests/engine_model.py) for the seeds the GPU tier runs -- nothing here is measured on a card.  CPU only."""
import numpy as np
import pytest

import engine_model as EM
import sequence_script as SS
from engines import K5, N1
from oracle_replay import np_states

MAX_STEPS = K5['max_steps']
REFILL_PERIOD = 8                                    # steps between two refills of the look-ahead rings
# the engines differ in three ways that move an episode: the plain 5 x 5 batch (whatever its frames), the pool with two menus, and 8 x 8
DYNAMICS = [(k, s, g) for k, s, g in SS.RUNS if k in ('state_manual', 'state_auto_pool_menus') or s == 8]


def test_circuit_is_eulerian():
    for seed in range(5):
        for n in (1, 2, 5, len(SS.MUTATORS)):
            tour = SS.circuit(n, np.random.RandomState(seed))
            assert len(tour) == n * n + 1 and tour[0] == tour[-1] == 0
            assert len(set(zip(tour, tour[1:]))) == n * n


def test_a_script_is_a_function_of_its_arguments():
    a, b = SS.script_of('state_auto_pool_menus', 2), SS.script_of('state_auto_pool_menus', 2)
    assert [n for n, _ in a] == [n for n, _ in b]
    for (_, x), (_, y) in zip(a, b):
        assert sorted(x) == sorted(y) and all(np.array_equal(x[k], y[k]) for k in x)
    plain = SS.script_of('state_manual', 2)                       # the pool changes one flag of the sample ops and nothing else
    assert [n for n, _ in a] == [n for n, _ in plain]
    assert all(x['pooled'] and not y['pooled'] for (n, x), (_, y) in zip(a, plain) if n == 'sample')
    assert [n for n, _ in SS.script_of('state_manual', 0)] != [n for n, _ in plain]


@pytest.mark.parametrize('gap', sorted(SS.SEEDS))
def test_every_ordered_pair_occurs_and_the_script_has_its_shape(gap):
    ops = SS.script_of('state_manual', gap)
    names = [n for n, _ in ops]
    assert names[0] == 'reset' and names[-1] == 'steps' and len(ops[-1][1]['actions']) == 2 * MAX_STEPS + 3
    tokens = SS.tokens_of(ops, MAX_STEPS)
    n = len(SS.MUTATORS)
    assert SS.unbroken_pairs(tokens, gap) == {(a, b) for a in range(n) for b in range(n)}
    # a segment of max_steps + 2 steps after every K-th op, the gap's steps after every other one, no other steps
    count = 0
    for i, t in enumerate(tokens):
        if t in ('segment', 'gap'):
            assert tokens[i - 1] not in ('segment', 'gap') and (count % SS.K_OPS == 0) == (t == 'segment')
        else:
            count += 1
            if i + 1 < len(tokens):
                assert (tokens[i + 1] in ('segment', 'gap')) == (count % SS.K_OPS == 0 or gap > 0)
    assert {len(a['actions']) for nm, a in ops[:-1] if nm == 'steps'} == ({MAX_STEPS + 2, gap} if gap else {MAX_STEPS + 2})
    # every checkpoint is loaded, two mutators after its save
    muts = [i for i, nm in enumerate(names) if nm in SS.MUTATORS]
    loads = [i for i, nm in enumerate(names) if nm == 'ckpt_load']
    saves = [i for i, nm in enumerate(names) if nm == 'ckpt_save']
    assert len(loads) == len(saves) >= n
    for s, l in zip(saves, loads):
        assert len([i for i in muts if s < i < l]) <= SS.CKPT_LOAD_AFTER
        assert len([i for i in muts if s < i < l]) == SS.CKPT_LOAD_AFTER or l > muts[-1]
    # the rows of the loads: a fork, a drawn order, no part, past the bank, never saved
    saved = set()
    for nm, a in ops:
        if nm == 'save':
            r = a['rows']
            used = r[(r >= 0) & (r < SS.CAP)]
            assert len(set(used.tolist())) == len(used) and used.max() < SS.NEVER[0] and (r >= SS.CAP).sum() == 1 and (r < 0).any()
            saved |= set(used.tolist())
        elif nm in ('load_stream', 'load_episode'):
            r = a['rows']
            good = r[np.isin(r, sorted(saved))]
            assert np.bincount(good).max() >= N1 // 7 and len(set(good.tolist())) >= N1 // 3
            assert (r == -1).any() and (r >= SS.CAP).any() and ((r >= SS.NEVER[0]) & (r < SS.NEVER[1])).any()


@pytest.mark.parametrize('kind,size,gap', DYNAMICS)
def test_conditions_from_the_model_alone(kind, size, gap):
    ops = SS.script_of(kind, gap)
    model, _ = EM.model_for(kind, size, *np_states(N1, SS.BASE))
    model.snapshot_reserve(SS.CAP)
    pending, resets, doubles, commits = [], np.zeros(N1, np.int64), 0, 0
    for i, (name, args) in enumerate(ops):
        tag = SS.describe(ops, i)
        if 'mask' in args:
            k = int(np.count_nonzero(args['mask']))
            assert 4 * k >= N1 and 4 * (N1 - k) >= N1, tag
        before = model.expected()['desired'].copy() if name == 'imagine_commit' else None
        out = EM.apply(model, name, args, pending)
        if name == 'steps':
            done = out['done']
            resets += done.sum(axis=0)
            if len(done) >= MAX_STEPS + 2:
                assert done.any(), tag
            for e in range(N1):
                doubles += int((np.diff(np.flatnonzero(done[:, e])) < REFILL_PERIOD).sum())
        elif name in ('load_stream', 'load_episode'):
            r = args['rows']
            assert 3 * len(out['good']) >= N1 and int((r >= 0).sum()) - len(out['good']) >= 1, tag
        elif name == 'imagine_commit':
            rows = out['rows']
            assert (model.expected()['desired'][rows] != before[rows]).any(), tag
            commits += 1
    assert not pending and commits >= len(SS.MUTATORS)
    assert resets.min() >= 2
    # an env that finishes twice fewer than REFILL_PERIOD steps apart does so within one period wherever the period's edge falls between ops only if
    # the edge misses it: three such events at the least, so that the case does not hang on one alignment
    assert doubles >= 3, doubles
    assert model.counters[EM.COUNTERS[-1]] > 0 and model.counters[2] > 0
