"""GPU tier of cw_reach where its loops take a SECOND ROUND: a search large enough that cw_reach_scan_kernel's lanes sum several chunk counts each (more
than 1 024 chunks), that the workgroups of cw_reach_count_kernel / cw_reach_scatter_kernel meet a second chunk (more chunks than their grid), and that the
lanes of cw_reach_start_kernel / cw_reach_settle_kernel / cw_reach_walk_kernel take a second start row (more start rows than their lanes).  The shape is
derived from the card and the header's constants: M0 start rows tiled from the twelve 5 x 5 envs the reach tests share -- the smallest multiple of 12 above
the start-row lanes, enlarged if the card is so small that level 2 would not pass 1 024 chunks --, depth 3, max_rows 2^22.  One engine, two reach() /
reach_async() pairs at that size and the small searches they are compared with; every comparison is exact.  No timing is asserted."""
import time

import numpy as np
import pytest
import torch

from engines import n_cu
from reach_check import CHUNK, rows_of
from records_gpu import dev as _dev, tiled_rows
from seen_check import REACH_N, reach_reference
from test_reach_async import _both, _clean, _host, _plans_hold, _start_engine

pytestmark = pytest.mark.gpu

DEPTH, MAX_ROWS = 3, 1 << 22
SMALL_ROWS = 1 << 10


def _chunks(frontier):
    return (rows_of(int(frontier)) + CHUNK - 1) // CHUNK


def _small(env, eo=None):
    """reach_async(3) of the engine's own twelve records (eo: their env_of) into the small workspace, as numpy"""
    r = env.reach_async(DEPTH, env.hdr, env.slot_pos, _dev(np.arange(REACH_N) if eo is None else eo, np.int32), max_rows=SMALL_ROWS)
    torch.cuda.synchronize()
    _clean(env)
    return _host(r)


class _Search:
    """the engine, the shape, the small searches and -- run on first use, once, a failure kept and raised again -- the pair of calls at full size"""

    def __init__(self):
        from gym_craftingworld_amd import _lib as L
        lib = L.load()
        self.rows = self.first = self.failed = None
        self.seconds = 0.0
        self.env = _start_engine(5)
        try:
            self._prepare(lib)
        except BaseException:
            self.release()
            raise

    def _prepare(self, lib):
        env = self.env
        env.seen_reserve(1 << 14)
        self.small = _small(env)                                                   # tests/test_reach_async.py pins this shape to the oracle
        alone = [_small(env, np.where(np.arange(REACH_N) == e, e, -1)) for e in range(REACH_N)]
        self.alone = np.stack([a['frontier'] for a in alone]).astype(np.int64)     # [env, level]: what each env's start row brings to a level
        self.lanes = 256 * lib.cwh_reach_grid_of(MAX_ROWS, n_cu())                 # of the start, settle and walk kernels
        self.chunk_grid = lib.cwh_reach_grid_of(256 * _chunks(MAX_ROWS), n_cu())   # workgroups of count and scatter
        k = self.lanes // REACH_N + 1
        while _chunks(k * int(self.small['frontier'][1])) <= 1024:                 # (a card with few CUs: the scan's second round decides)
            k += 1
        self.k, self.M0 = k, REACH_N * k
        env.seen_reserve(1 << 23)
        env.reach_reserve(MAX_ROWS, DEPTH)
        self.rows = tiled_rows(env, self.M0)

    def pair(self):
        if self.failed is not None:
            raise self.failed
        if self.first is None:
            t0 = time.perf_counter()
            try:
                self.first = _both(self.env, DEPTH, *self.rows, max_rows=MAX_ROWS, engine=True)[1]
            except BaseException as e:  # noqa: BLE001
                self.failed = e
                raise
            self.seconds = time.perf_counter() - t0
        return self.first

    def release(self):
        self.rows = self.first = None
        self.env.reach_reserve(0, 1)
        self.env.seen_reserve(0)
        self.env.close()
        torch.cuda.empty_cache()


@pytest.fixture(scope='module')
def search():
    torch.cuda.reset_peak_memory_stats()
    s = None
    try:
        s = _Search()
        yield s
        print('\ntest_reach_rounds: %d CUs, M0 = %d start rows, frontiers %s, first pair %.2f s, reach_bytes = %d, torch.cuda.max_memory_allocated() = %d'
              % (n_cu(), s.M0, None if s.first is None else s.first['frontier'].tolist(), s.seconds, s.env.reach_bytes, torch.cuda.max_memory_allocated()))
    finally:
        if s is not None:
            s.release()
        torch.cuda.empty_cache()


def test_the_shape_takes_every_loop_into_its_second_round(search):
    """what makes this file meaningful, asserted and not assumed: level 2 compacts more chunks than the scan has lanes and than count and scatter have
    workgroups; there are more start rows than the start-row kernels have lanes; solved and unsolved rows lie in the second round; the search ran all three
    levels with a clean set"""
    s = search
    got = s.pair()
    n_chunks = _chunks(got['frontier'][1])
    assert n_chunks > max(1024, s.chunk_grid), (n_chunks, s.chunk_grid)
    assert s.M0 > s.lanes and s.M0 % REACH_N == 0 and s.M0 <= MAX_ROWS
    late = got['distance'][s.lanes:]
    assert (late > 0).any() and (late == -1).any()
    assert got['searched_depth'][0] == DEPTH and (got['frontier'] <= MAX_ROWS).all()
    _clean(s.env)


def test_against_the_cpu_oracle(search):
    """the independent reference: row j's distance is that of the pure CPU breadth-first search over the oracle from env j % 12's start state, and frontier 0
    holds every start row"""
    s = search
    got = s.pair()
    ref = reach_reference(5, DEPTH)[2]['distance']
    assert (ref > 0).any() and (ref < 0).any()
    assert np.array_equal(got['distance'], np.tile(ref, s.k))
    assert got['frontier'][0] == s.M0 == len(got['distance'])


def test_against_the_small_search(search):
    """k = M0 / 12 copies of the twelve start rows give the small search's result k times over: plan, first_action and distance repeat, every frontier and
    the states held are k times the small search's.  EXACTLY, because (1) a start row is searched in a group of its own -- its row number is word 0 of every
    key it inserts, and a hit bids for its own start row only --, so which states a start row meets does not depend on the other rows; and (2) the order
    among a start row's own states does not depend on them either, by induction over the levels: frontier 0 holds the start rows in row order; if the
    states of one start row stand in frontier d - 1 in the same relative order as in the small search, then so do their successor rows a * Fp + j (Fp > j:
    the order is lexicographic in (action, position), and positions keep their relative order), the set's smallest-row rule picks the same winner among
    equal keys of the group, the stable compaction keeps the winners' order, and the smallest solving row names the same (action, state).  So each copy's
    links, walked back, spell the small search's plan.  A chunk lost, doubled or misplaced in any round changes `frontier` or `states`; a start row served by
    the wrong round changes `plan` or `distance`."""
    s = search
    got, small, k = s.pair(), s.small, s.k
    assert small['frontier'].tolist() == s.alone.sum(axis=0).tolist() and int(small['frontier'][0]) == REACH_N      # (1), on the small search itself
    assert np.array_equal(got['plan'], np.tile(small['plan'], (1, k)))
    assert np.array_equal(got['first_action'], np.tile(small['first_action'], k))
    assert np.array_equal(got['distance'], np.tile(small['distance'], k))
    assert got['frontier'].astype(np.int64).tolist() == (k * small['frontier'].astype(np.int64)).tolist()
    assert int(got['states'][0]) == k * int(small['states'][0])


def test_the_plans_through_simulate(search):
    """the [3, M0] plan through simulate() on the same records: every solved row, those of the second round included, ends done by success at
    length == distance"""
    s = search
    got = s.pair()
    dist = _plans_hold(s.env, got, *s.rows)
    assert (dist[s.lanes:] > 0).any() and (dist[:s.lanes] > 0).sum() >= 2 * (s.k - 1)


def test_rows_that_take_no_part_in_the_second_round(search):
    """a second pair of calls with three env_of entries that name no env -- row lanes + 1 (-1), the last row (num_envs) and row 5 (-7): they report -1,
    zeros and 0, frontier 0 is three rows short, every level misses exactly what those rows' envs bring in the small search, expand_skipped does not move,
    and every other row is as in the first pair"""
    s = search
    first = s.pair()
    env, M0 = s.env, s.M0
    out_rows = np.array([s.lanes + 1, M0 - 1, 5])
    eo = np.arange(M0, dtype=np.int64) % REACH_N
    eo[out_rows] = [-1, REACH_N, -7]
    skipped = env.expand_skipped
    _, got = _both(env, DEPTH, s.rows[0], s.rows[1], _dev(eo, np.int32), max_rows=MAX_ROWS, engine=True)
    assert env.expand_skipped == skipped
    assert (got['distance'][out_rows] == -1).all() and (got['plan'][:, out_rows] == 0).all() and (got['first_action'][out_rows] == 0).all()
    gone = s.alone[out_rows % REACH_N].sum(axis=0)
    assert gone[0] == 3 and got['frontier'][0] == M0 - 3
    assert got['frontier'].astype(np.int64).tolist() == (first['frontier'].astype(np.int64) - gone).tolist()
    keep = np.ones(M0, bool)
    keep[out_rows] = False
    for f in ('distance', 'first_action'):
        assert np.array_equal(got[f][keep], first[f][keep]), f
    assert np.array_equal(got['plan'][:, keep], first['plan'][:, keep]) and got['searched_depth'][0] == DEPTH
