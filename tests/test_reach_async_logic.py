"""CPU tier: the numpy model of cw_reach's levels (tests/reach_check.py) and the checker of its GPU tests.  The model, driven by the CPU oracle, reproduces
seen_check.reference_reach on the start rows the reach tests share; its pieces -- the padded row numbering, the chunked compaction, the stop rule -- are
held against their plain definitions; and check_reach_call passes a correct result and catches each planted fault."""
import numpy as np
import pytest

from reach_check import (CHUNK, FAULTS, WAVE, as_reference, check_reach_call, compact, model_reach, padded, row_of, rows_of, run_model)
from records_fixtures import SENT, snap, world
from seen_check import REACH_MAX_STEPS, REACH_N, reach_reference

DEPTH = 10


# ------------------------------------------------------------------------------------------------------------------------------ 1. against the reference
@pytest.mark.parametrize('size', [5, 8])
def test_the_model_reproduces_the_reference(size):
    """12 start rows, depth 10: the distances, the frontier sizes (test_reach.py compares the first three with the card: the reference, like the model here,
    merges slot orders by its canonical encoding, the card does not), the states met and searched_depth; the plans are as long as the distances say"""
    dense, inits, ref = reach_reference(size, DEPTH)
    r = model_reach(dense, inits, DEPTH, dict(size=(size, size), max_steps=REACH_MAX_STEPS), 1 << 16)
    assert np.array_equal(r['distance'], ref['distance']) and (r['distance'] > 0).sum() * 4 >= REACH_N
    assert r['frontier'][:3].tolist() == ref['frontier'][:3] and r['frontier'][:len(ref['frontier'])].tolist() == ref['frontier']
    assert r['searched_depth'] == ref['searched_depth'] == DEPTH and r['states'] == ref['states']
    assert np.array_equal((r['plan'] != 0).sum(axis=0) <= np.maximum(r['distance'], 0), np.ones(REACH_N, bool))
    check_reach_call(r, _buffers(r), SENT)


def test_max_rows_60_stops_the_model_at_level_3():
    dense, inits, ref = reach_reference(5, DEPTH)
    assert ref['frontier'][:4] == [12, 35, 55, 69]
    r = model_reach(dense, inits, DEPTH, dict(size=(5, 5), max_steps=REACH_MAX_STEPS), 60)
    assert r['searched_depth'] == 3 and r['frontier'].tolist() == [12, 35, 55] + [0] * 7
    assert np.array_equal(r['distance'], np.where((ref['distance'] > 0) & (ref['distance'] <= 3), ref['distance'], -1))
    check_reach_call(r, _buffers(r), SENT)
    r69 = model_reach(dense, inits, 4, dict(size=(5, 5), max_steps=REACH_MAX_STEPS), 69)                  # exactly max_rows fresh rows is not above it
    assert r69['searched_depth'] == 4 and r69['frontier'].tolist() == [12, 35, 55, 69]


def test_rows_that_take_no_part():
    dense, inits, ref = reach_reference(5, DEPTH)
    part = np.arange(REACH_N) % 3 != 1
    r = model_reach(dense, inits, 6, dict(size=(5, 5), max_steps=REACH_MAX_STEPS), 1 << 16, part=part)
    want = np.where(part & (ref['distance'] > 0) & (ref['distance'] <= 6), ref['distance'], -1)
    assert np.array_equal(r['distance'], want) and r['frontier'][0] == part.sum() and (r['plan'][:, ~part] == 0).all()


# ------------------------------------------------------------------------------------------------------------------------------ 2. the pieces
@pytest.mark.parametrize('F', [1, 2, 63, 64, 65, 700])
def test_the_padded_numbering_keeps_the_order(F):
    rows = np.array([[row_of(a, j, F) for j in range(F)] for a in range(6)])
    assert np.array_equal(np.argsort(rows.reshape(-1), kind='stable'), np.arange(6 * F))               # the order of a * F + j
    assert rows.max() < rows_of(F) == 6 * padded(F) and padded(F) % WAVE == 0 and 0 <= padded(F) - F < WAVE
    assert (rows // WAVE * WAVE // padded(F) == rows // padded(F)).all()                                # a wave's first row is of the same action
    assert rows_of(0) == 0


@pytest.mark.parametrize('n', [0, 1, 15, 16, 17, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 77])
def test_the_chunked_compaction_is_flatnonzero(n):
    for density in (0.0, 0.03, 0.5, 1.0):
        flags = np.random.RandomState(n + int(100 * density)).rand(n) < density
        places, counts, ahead = compact(flags)
        assert np.array_equal(places, np.flatnonzero(flags))
        assert len(counts) == (n + CHUNK - 1) // CHUNK and counts.sum() == flags.sum()
        assert np.array_equal(ahead, np.cumsum(counts) - counts)
    places, _, _ = compact(np.ones(n, bool), chunk=64, lanes=4)                                         # another shape of the same rule
    assert np.array_equal(places, np.arange(n))


# ------------------------------------------------------------------------------------------------------------------------------ 3. the checker
TABLE_STATES, TABLE_STARTS, TABLE_DEPTH = 2000, 9, 6


def _table(seed=11):
    """a successor table instead of a world: state s under action a becomes nxt[s, a], pays with probability 1 / 500 and is done with 11 / 20 (the frontiers
    grow to a few hundred states, the nine start rows are solved at levels 4 to 6 or not at all)"""
    r = np.random.RandomState(seed)
    nxt, pays, ends = r.randint(0, TABLE_STATES, (TABLE_STATES, 6)), r.rand(TABLE_STATES, 6) < 0.002, r.rand(TABLE_STATES, 6) < 0.55
    # ... and one TIE, where the frontier's order decides: start row 0 (state 0) reaches states 1 .. 6, of which 1 and 2 both pay under action 2 -- the
    # smaller row, state 1's, wins, and the plan starts with action 0
    nxt[0], pays[0], ends[0] = np.arange(1, 7), False, False
    pays[1:7], ends[1:7] = False, False
    pays[1, 2] = pays[2, 2] = True
    return nxt, pays, ends


def _table_search(faults=(), max_rows=1 << 12, tile=1, **model_kw):
    """tile: the nine start rows `tile` times over, row j is base row j % 9; model_kw: run_model's chunk and chunk_grid"""
    nxt, pays, ends = _table()

    def successors(front):
        s = np.asarray(front)
        keys = np.zeros((6 * len(s), 2), np.uint32)
        keys[:, 1] = nxt[s].T.reshape(-1)
        return pays[s].T, ends[s].T | pays[s].T, keys, nxt[s].T.reshape(-1)
    starts = np.tile(np.arange(TABLE_STARTS) * 7, tile)
    part = np.tile(np.arange(TABLE_STARTS) != 4, tile)
    keys = np.zeros((TABLE_STARTS * tile, 2), np.uint32)
    keys[:, 1] = starts
    return run_model(part, keys, starts, successors, max_rows, TABLE_DEPTH, faults, **model_kw)


def _buffers(r, **changed):
    r = dict(as_reference(r), **changed)
    return dict(distance=r['distance'].astype(np.int32), plan=r['plan'].astype(np.uint8), first_action=r['first_action'].astype(np.uint8),
                frontier=r['frontier'].astype(np.int32), searched_depth=np.array([r['searched_depth']], np.int32), states=np.array([r['states']], np.int64))


def _brute_table():
    """the distances of the table search by plain breadth-first search per start row, a dict of depths"""
    nxt, pays, ends = _table()
    out = []
    for s0 in np.arange(TABLE_STARTS) * 7:
        seen, front, found = {int(s0)}, [int(s0)], -1
        for d in range(1, TABLE_DEPTH + 1):
            if any(pays[s].any() for s in front):
                found = d
                break
            new = []
            for a in range(6):
                for s in front:
                    t = int(nxt[s, a])
                    if not ends[s, a] and not pays[s, a] and t not in seen:
                        seen.add(t)
                        new.append(t)
            front = new
        out.append(found)
    return np.array(out)


def test_a_correct_result_passes_and_is_the_breadth_first_one():
    r = _table_search()
    want = _brute_table()
    want[4] = -1
    assert np.array_equal(r['distance'], want) and (want > 0).sum() >= 4 and len(set(want[want > 0].tolist())) >= 3 and (want < 0).sum() >= 2
    dense, inits = world()
    engine = snap(dense, inits)
    check_reach_call(r, _buffers(r), SENT, engine, {k: v.copy() for k, v in engine.items()})
    stopped = _table_search(max_rows=40)
    assert stopped['searched_depth'] < TABLE_DEPTH and (stopped['frontier'][stopped['searched_depth']:] == 0).all()
    check_reach_call(stopped, _buffers(stopped), SENT)


FAULT_SHAPE = {'chunk_round_lost': dict(chunk=256, chunk_grid=2)}          # the launch a fault needs to show: chunks of 256 rows, two workgroups


@pytest.mark.parametrize('fault', FAULTS)
def test_a_planted_fault_is_caught(fault):
    """a swapped pair in the frontier order; a solved row that stays in the search, so that a later hit is accepted for it; a done row inserted; a link off by
    one; a nonzero behind a plan's end; the chunks beyond the first grid-stride round of count and scatter lost"""
    good, bad = _table_search(), _table_search(faults=(fault,), **FAULT_SHAPE.get(fault, {}))
    with pytest.raises(AssertionError):
        check_reach_call(good, _buffers(bad), SENT)


def test_what_else_the_checker_catches():
    r = _table_search()
    j = int(np.flatnonzero(r['distance'] > 1)[0])
    cases = []
    d = r['distance'].copy()
    d[j] += 1
    cases.append(dict(distance=d))
    f = r['frontier'].copy()
    f[2] += 1
    cases.append(dict(frontier=f))
    cases.append(dict(searched_depth=r['searched_depth'] - 1))
    p = r['plan'].copy()
    p[0, j] = (p[0, j] + 1) % 6
    cases.append(dict(plan=p))                                                                          # (first_action no longer plan[0], and another plan)
    cases.append(dict(plan=p, first_action=p[0].copy()))
    cases.append(dict(states=r['states'] + 1))
    for c in cases:
        with pytest.raises(AssertionError):
            check_reach_call(r, _buffers(r, **c), SENT)
    b = _buffers(r)
    b['distance'].view(np.uint8).reshape(-1, 4)[4] = SENT                                               # a row that takes no part must be written too
    with pytest.raises(AssertionError, match='sentinel'):
        check_reach_call(r, b, SENT)
    b = _buffers(r)
    b['plan'][TABLE_DEPTH - 1, 4] = SENT
    with pytest.raises(AssertionError, match='sentinel'):
        check_reach_call(r, b, SENT)
    dense, inits = world()
    engine = snap(dense, inits)
    after = {k: v.copy() for k, v in engine.items()}
    after['counters'][7] += 1                                                                           # a skipped start row counted: cw_reach does not
    with pytest.raises(AssertionError, match='counters'):
        check_reach_call(r, _buffers(r), SENT, engine, after)
    with pytest.raises(ValueError):
        check_reach_call(r, dict(_buffers(r), frontier=np.zeros(3, np.int32)), SENT)


# ------------------------------------------------------------------------------------------------------------------------------ 4. tiled start rows
TILE, TILE_CHUNK = 7, 256


def _tiling_of(base, k):
    """what a search over the base start rows k times over must give if start rows are searched apart and the order within a start row's own states is
    kept: every per-row output repeats, every count is k times the base's (the comparison tests/test_reach_rounds.py makes on the card)"""
    return dict(distance=np.tile(base['distance'], k), plan=np.tile(base['plan'], (1, k)), first_action=np.tile(base['first_action'], k),
                frontier=k * base['frontier'], searched_depth=base['searched_depth'], states=k * base['states'])


def test_tiled_start_rows_give_the_tiling_of_the_base_result():
    """the table search once with its nine start rows and once with them seven times over, in chunks of 256 rows so that the tiled levels span many chunks:
    distance, plan and first_action repeat (the tie of start row 0 included), frontier and states are seven times the base's"""
    base, tiled = _table_search(chunk=TILE_CHUNK), _table_search(tile=TILE, chunk=TILE_CHUNK)
    assert rows_of(int(tiled['frontier'].max())) > 8 * TILE_CHUNK and base['plan'][0, 0] == 0 and base['distance'][0] == 2      # (the tie: action 0 first)
    want = _tiling_of(base, TILE)
    for f in ('distance', 'plan', 'first_action', 'frontier'):
        assert np.array_equal(tiled[f], want[f]), f
    assert tiled['states'] == want['states'] and tiled['searched_depth'] == want['searched_depth'] == TABLE_DEPTH
    check_reach_call(want, _buffers(tiled), SENT)
    same_chunks = _table_search(tile=TILE)                                                                # the chunk size does not enter the result
    check_reach_call(same_chunks, _buffers(tiled), SENT)


def test_a_lost_chunk_round_breaks_the_tiling():
    """'chunk_round_lost' with four workgroups: the fresh rows of every chunk from the fifth on never reach the next frontier.  The base search, whose levels
    fit the four chunks' 1 024 rows or lose less, no longer tiles into the faulted search: the frontier is smaller than seven times the base's; and
    check_reach_call against the unfaulted model names the frontier or the distance"""
    base, good = _table_search(chunk=TILE_CHUNK), _table_search(tile=TILE, chunk=TILE_CHUNK)
    bad = _table_search(tile=TILE, chunk=TILE_CHUNK, chunk_grid=4, faults=('chunk_round_lost',))
    want = _tiling_of(base, TILE)
    lvl = int(np.flatnonzero(bad['frontier'] != want['frontier'])[0])
    assert lvl >= 1 and bad['frontier'][lvl] < want['frontier'][lvl] and (bad['frontier'][:lvl] == want['frontier'][:lvl]).all()
    assert rows_of(int(want['frontier'][lvl - 1])) > 4 * TILE_CHUNK                                      # (the level whose compaction had a fifth chunk)
    assert bad['states'] < want['states']
    with pytest.raises(AssertionError, match='frontier|distance'):
        check_reach_call(good, _buffers(bad), SENT)
    unfaulted = _table_search(tile=TILE, chunk=TILE_CHUNK, chunk_grid=4)                                  # the grid alone changes nothing: the fault is opt-in
    check_reach_call(good, _buffers(unfaulted), SENT)
