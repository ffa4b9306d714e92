"""What "a reach_async call did exactly what it should" means for cw_reach, said once.  ReachModel is one search in numpy as the kernels run it, level by
level, with the SUCCESSORS TAKEN AS GIVEN (which rows pay max_steps, which are done, and their keys): the padded row numbering a * Fp + j, the bids by
smallest row and the settle rule, the groups of the insert, the chunked count / scan / scatter, the stop rule, the links and the walk-back.  run_model() drives
it over any successor function -- the CPU oracle (oracle_successors) or a table (the logic tests plant faults on one).  check_reach_call() compares what a
call wrote with a reference result: every output exactly, into buffers every byte of which held the sentinel before (cw_reach writes every element it is
given, the rows that take no part included, so no sentinel may be left), and the engine before and after the call (masked_check.take() snapshots: nothing may
have changed).  Pure CPU: numpy arrays in, no GPU.  A plain module, not a fixture; tests/test_reach_async_logic.py tests the comparison itself."""
import numpy as np

from oracle_replay import same
from records_check import DENSE, encode, oracle_simulate
from seen_check import SeenModel, key_of

WAVE, CHUNK, NONE = 64, 4096, 2 ** 31 - 1
FAULTS = ('swap_frontier', 'solved_row_stays', 'done_inserted', 'link_off_by_one', 'plan_tail', 'chunk_round_lost')


def padded(F):
    return (F + WAVE - 1) // WAVE * WAVE


def rows_of(F):
    """rows of a level over F states: six actions times F rounded up to a wavefront"""
    return 6 * padded(F)


def row_of(a, j, F):
    """THE ROW of action a on frontier state j: a * Fp + j -- the order of a * F + j, and no wave of 64 rows holds two actions"""
    return a * padded(F) + j


def compact(flags, chunk=CHUNK, lanes=256, lost_from=None):
    """the kernels' stable compaction of the set flags: per chunk of `chunk` rows a count (every lane of `lanes` takes chunk // lanes consecutive flags), one
    scan over the chunk counts, and per chunk again the place of each set flag = what lies ahead of the chunk + the prefix of the lanes ahead + its rank in
    its lane -> (places int64 [n]: places[k] is the row that lands at k, the chunk counts, what lies ahead of each chunk).  lost_from (the fault
    'chunk_round_lost'): the set flags of every chunk at or above that count are ignored -- count and scatter launched with lost_from workgroups whose
    grid-stride loop never takes its second round"""
    flags = np.asarray(flags).astype(bool)
    n = len(flags)
    n_chunks = (n + chunk - 1) // chunk
    per = chunk // lanes
    grid = np.zeros(n_chunks * chunk, bool)
    grid[:n] = flags                                                   # (rows at or above n are cleared, whatever the buffer holds)
    if lost_from is not None:
        grid[int(lost_from) * chunk:] = False
    lane_counts = grid.reshape(n_chunks, lanes, per).sum(axis=2)
    counts = lane_counts.sum(axis=1)
    ahead = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64) if n_chunks else np.zeros(0, np.int64)
    places = np.full(int(counts.sum()), -1, np.int64)
    for c in range(n_chunks):
        lane_ahead = np.concatenate([[0], np.cumsum(lane_counts[c])[:-1]])
        for t in np.flatnonzero(lane_counts[c]):
            at = ahead[c] + lane_ahead[t]
            r0 = c * chunk + t * per
            for b in np.flatnonzero(grid[r0:r0 + per]):
                places[at] = r0 + b
                at += 1
    return places, counts.astype(np.int64), ahead


class ReachModel:
    """one search.  part: bool [M0], which start rows take part.  start(keys) and then level(d, hit, done, keys) for d = 1, 2, ... return the next frontier as
    indices into the rows handed in (start rows; then successors in the order a * F + j), which the caller gathers; result() walks the plans back.
    faults: names of FAULTS to plant.  chunk_grid: the workgroups count and scatter are launched with, which only 'chunk_round_lost' reads."""

    def __init__(self, part, max_rows, max_depth, faults=(), chunk=CHUNK, chunk_grid=1):
        self.part = np.asarray(part).astype(bool)
        self.M0, self.max_rows, self.D, self.faults, self.chunk = len(self.part), int(max_rows), int(max_depth), tuple(faults), chunk
        assert set(self.faults) <= set(FAULTS)
        self.lost_from = int(chunk_grid) if 'chunk_round_lost' in self.faults else None
        self.seen = SeenModel()
        self.dist = np.full(self.M0, -1, np.int64)
        self.sol = np.zeros(self.M0, np.int64)
        self.active = self.part.copy()
        self.sizes = np.zeros(self.D + 1, np.int64)
        self.searched, self.stopped = self.D, False
        self.links = []                                                # links[k - 1]: parent << 3 | action of every state of frontier k
        self.f_start = np.zeros(0, np.int64)

    def _keys(self, keys, group):
        k = np.array(keys, dtype=np.uint32).reshape(len(group), -1)
        k[:, 0] = (np.asarray(group).astype(np.int64) & 0xFFFFFFFF).astype(np.uint32)
        return k

    def start(self, keys):
        """the set is cleared; the participating start rows go in with group = their row number and form frontier 0 in row order"""
        self.seen.clear()
        rows = np.arange(self.M0, dtype=np.int64)
        self.seen.insert(self._keys(keys, rows), self.part)
        places, _, _ = compact(self.part, self.chunk, lost_from=self.lost_from)
        assert self.lost_from is not None or np.array_equal(places, np.flatnonzero(self.part))
        self.f_start = places
        self.sizes[0] = len(places)
        return places

    def level(self, d, hit, done, keys):
        """level d over the frontier in hand.  hit, done: bool [6, F]; keys: [6 * F, words] in the order a * F + j (word 0 is replaced by the group)"""
        F = len(self.f_start)
        assert self.sizes[d - 1] == F and not self.stopped and 1 <= d <= self.D
        hit, done = np.asarray(hit).astype(bool).reshape(6, F), np.asarray(done).astype(bool).reshape(6, F)
        Fp, n = padded(F), rows_of(F)
        a_of, j_of = np.arange(n) // max(Fp, 1), np.arange(n) % max(Fp, 1)
        real = j_of < F                                                # rows j >= F of an action take no part
        flat = np.where(real, a_of * F + np.minimum(j_of, max(F - 1, 0)), 0)       # the row's place in the order a * F + j
        assert np.array_equal(flat[real], np.arange(6 * F))           # the padded numbering keeps that order
        start = np.where(real, self.f_start[np.minimum(j_of, max(F - 1, 0))] if F else 0, 0)
        # expansion: a row whose reward is max_steps bids for its start row with its row number, while that start row is active
        bid = np.full(self.M0, NONE, np.int64)
        counts = real & hit.reshape(-1)[flat]
        if 'solved_row_stays' not in self.faults:
            counts &= self.active[start]
        np.minimum.at(bid, start[counts], np.flatnonzero(counts))
        group = np.where(real & ~done.reshape(-1)[flat], start, -1)
        if 'done_inserted' in self.faults:
            group = np.where(real, start, -1)
        nxt = np.zeros(0, np.int64)
        if d < self.D:
            # the insert reads the BIDS, not dist: a start row solved in this level takes its successors out of it
            g = group.copy()
            if 'solved_row_stays' not in self.faults:
                g[(g >= 0) & (bid[np.maximum(g, 0)] != NONE)] = -1
            k = np.zeros((n, np.asarray(keys).reshape(6 * F, -1).shape[1] if F else 1), np.uint32)
            if F:
                k[real] = np.asarray(keys).reshape(6 * F, -1)
            fresh, _ = self.seen.insert(self._keys(k, np.maximum(g, 0)), g >= 0)
            places, counts_c, ahead = compact(fresh, self.chunk, lost_from=self.lost_from)
            assert (self.lost_from is not None or np.array_equal(places, np.flatnonzero(fresh))) and counts_c.sum() == len(places)
            if len(places) > self.max_rows:                            # the stop rule: searched_depth = d, every later level is a no-op
                self.searched, self.stopped = d, True
                places = places[:0]
            if 'swap_frontier' in self.faults and len(places) >= 2:      # the first fresh row changes places with the next one of its start row (or its neighbour)
                mates = np.flatnonzero(start[places[1:]] == start[places[0]])
                k = 1 + int(mates[0]) if len(mates) else 1
                places = places.copy()
                places[[0, k]] = places[[k, 0]]
            self.sizes[d] = len(places)
            parent = j_of[places] + (1 if 'link_off_by_one' in self.faults else 0)
            self.links.append((parent << 3) | a_of[places])
            nxt = flat[places]
            next_start = start[places]
        # settle: one lane per start row turns a bid into dist, the solving link and inactive
        won = bid != NONE
        if 'solved_row_stays' not in self.faults:
            assert not (won & ~self.active).any()
        self.dist[won] = d
        self.sol[won] = ((bid[won] % max(Fp, 1)) << 3) | (bid[won] // max(Fp, 1))
        self.active &= ~won
        self.f_start = next_start if d < self.D else np.zeros(0, np.int64)
        return nxt

    def result(self):
        """the walk-back, one start row at a time: action sol & 7 at step dist, then along the links; zeros behind a plan's end and for -1 rows"""
        plan = np.zeros((self.D, self.M0), np.uint8)
        for s in np.flatnonzero(self.dist > 0):
            L, link = int(self.dist[s]), int(self.sol[s])
            for lvl in range(L, 0, -1):
                if lvl < L:
                    cur = link >> 3
                    link = int(self.links[lvl - 1][cur]) if cur < len(self.links[lvl - 1]) else 0
                plan[lvl - 1, s] = link & 7
            if 'plan_tail' in self.faults and L < self.D:
                plan[L, s] = 3
        return dict(distance=self.dist.copy(), plan=plan, first_action=plan[0].copy(), frontier=self.sizes[:self.D].copy(), searched_depth=self.searched,
                    states=len(self.seen))


def run_model(part, start_keys, payload, successors, max_rows, max_depth, faults=(), chunk=CHUNK, chunk_grid=1):
    """a whole search.  payload: anything indexable by an int array, one entry per start row; successors(payload of the frontier) -> (hit [6, F], done [6, F],
    keys [6 * F, words], payload of the 6 * F successors in the order a * F + j) -> ReachModel.result()"""
    m = ReachModel(part, max_rows, max_depth, faults, chunk, chunk_grid)
    front = payload[m.start(start_keys)]
    for d in range(1, max_depth + 1):
        if len(m.f_start) == 0:                                        # (an empty or stopped frontier: the remaining levels are no-ops)
            break
        hit, done, keys, succ = successors(front)
        front = succ[m.level(d, hit, done, keys)]
    return m.result()


class DenseStates:
    """dense states (records_check.DENSE) with their init grids, indexable by an int array like an array"""

    def __init__(self, dense, init_grids):
        self.dense, self.inits = {k: np.asarray(dense[k]) for k in DENSE}, np.asarray(init_grids)

    def __getitem__(self, idx):
        return DenseStates({k: v[idx] for k, v in self.dense.items()}, self.inits[idx])

    def __len__(self):
        return len(self.inits)

    def keys(self):
        h, p = encode(self.dense)
        return key_of(h, p, np.zeros(len(self)))


def oracle_successors(oracle_kw):
    """the successor function of run_model over the CPU oracle: one step of all six actions by records_check.oracle_simulate, as reference_reach takes it"""
    max_steps = int(oracle_kw['max_steps'])

    def successors(front):
        F = len(front)
        tiled = DenseStates({k: np.tile(v, (6,) + (1,) * (v.ndim - 1)) for k, v in front.dense.items()}, np.tile(front.inits, (6, 1, 1)))
        r = oracle_simulate(tiled.dense, tiled.inits, np.repeat(np.arange(6), F)[None, :], True, oracle_kw)
        succ = DenseStates({k: r[k] for k in DENSE}, tiled.inits)
        return (r['rewards'][0] == max_steps).reshape(6, F), np.asarray(r['dones'][0]).astype(bool).reshape(6, F), succ.keys(), succ
    return successors


def model_reach(dense, init_grids, max_depth, oracle_kw, max_rows, part=None, faults=()):
    """the model over the oracle from dense start states: what cw_reach finds from them (up to the slot orders the canonical encoding merges)"""
    st = DenseStates(dense, init_grids)
    part = np.ones(len(st), bool) if part is None else part
    return run_model(part, st.keys(), st, oracle_successors(oracle_kw), max_rows, max_depth, faults)


def as_reference(r):
    """a result of VecEnv.reach() (tensors, an int, a list) or of the model as numpy: distance int64 [M0], plan uint8 [D, M0], first_action uint8 [M0],
    frontier int64 [D] (zeros for the levels not run), searched_depth int, states int or None"""
    host = lambda t: t.cpu().numpy() if hasattr(t, 'cpu') else np.asarray(t)  # noqa: E731
    plan = host(r['plan']).astype(np.uint8)
    D = plan.shape[0]
    front = np.zeros(D, np.int64)
    f = host(r['frontier']).astype(np.int64).reshape(-1)
    front[:len(f)] = f[:D]
    states = r.get('states')
    return dict(distance=host(r['distance']).astype(np.int64), plan=plan, first_action=host(r['first_action']).astype(np.uint8), frontier=front,
                searched_depth=int(host(r['searched_depth']).reshape(-1)[0]), states=None if states is None else int(host(states).reshape(-1)[0]))


def check_reach_call(ref, got, sentinel, engine_before=None, engine_after=None):
    """Pure CPU.  cw_reach ran once.  ref: the result it should have left (as_reference takes reach()'s dict or the model's); got: the five output buffers
    as numpy -- distance int32 [M0], plan uint8 [D, M0], first_action uint8 [M0], frontier int32 [D], searched_depth int32 [1] -- and optionally 'states',
    as the call left buffers every byte of which held `sentinel` before.  Every element equals the reference, so none holds the sentinel: the rows that take
    no part are written too (-1, zeros).  Beyond the reference, what any result obeys: an action is 0 .. 5, first_action is plan[0], a plan is zeros behind
    its end and for -1 rows, a distance is -1 or 1 .. searched_depth, the frontier sizes are zeros from the first zero on and from searched_depth on.
    engine_before / engine_after: masked_check.take() snapshots (None, None: not compared): nothing changed, counters included."""
    ref = as_reference(ref)
    D, M0 = ref['plan'].shape
    dist, plan = np.asarray(got['distance']), np.asarray(got['plan'])
    first, front, searched = np.asarray(got['first_action']), np.asarray(got['frontier']), np.asarray(got['searched_depth'])
    if (dist.shape, plan.shape, first.shape, front.shape, searched.shape) != ((M0,), (D, M0), (M0,), (D,), (1,)):
        raise ValueError('the outputs hold %s, the reference %d rows and %d levels' % ((dist.shape, plan.shape, first.shape, front.shape, searched.shape), M0, D))
    for name, a in (('distance', dist), ('plan', plan), ('first_action', first), ('frontier', front), ('searched_depth', searched)):
        raw = np.ascontiguousarray(a).view(np.uint8).reshape(a.size, a.itemsize)
        left = np.flatnonzero((raw == sentinel).all(axis=1))
        assert len(left) == 0, '%s still holds the sentinel at %d elements, first %s' % (name, len(left), left[:8].tolist())
    rows = np.arange(M0)
    d = dist.astype(np.int64)
    s = int(searched[0])
    assert 1 <= s <= D, 'searched_depth = %d of %d levels' % (s, D)
    assert (plan <= 5).all(), 'an action above 5 in the plan'
    same('first_action == plan[0]', rows, first, plan[0])
    assert (((d == -1) | (d >= 1)) & (d <= s)).all(), 'a distance that is neither -1 nor 1 .. searched_depth = %d: %s' % (s, d[(d < -1) | (d == 0) | (d > s)][:8].tolist())
    behind = np.arange(D)[:, None] >= np.where(d > 0, d, 0)[None, :]
    bad = np.flatnonzero((plan != 0) & behind)
    assert len(bad) == 0, 'a nonzero behind a plan\'s end at (level, row) %s' % [(int(b // M0), int(b % M0)) for b in bad[:8]]
    f = front.astype(np.int64)
    z = np.flatnonzero(f == 0)
    assert (f >= 0).all() and (len(z) == 0 or (f[z[0]:] == 0).all()), 'frontier sizes after an empty level: %s' % f.tolist()
    assert s == D or (f[s:] == 0).all(), 'levels run behind searched_depth = %d: %s' % (s, f.tolist())
    same('distance', rows, d, ref['distance'])
    same('frontier', np.arange(D), f, ref['frontier'])
    assert s == ref['searched_depth'], 'searched_depth = %d, the reference %d' % (s, ref['searched_depth'])
    same('plan', rows, plan.T, ref['plan'].T)
    if 'states' in got and ref['states'] is not None:
        n = int(np.asarray(got['states']).reshape(-1)[0])
        assert n == ref['states'], 'the set holds %d keys, the reference %d' % (n, ref['states'])
    if engine_before is not None or engine_after is not None:
        if set(engine_before) != set(engine_after):
            raise ValueError('the snapshots hold different entries: %s' % sorted(set(engine_before) ^ set(engine_after)))
        for k in sorted(engine_before):
            same('after cw_reach: %s' % k, 0, engine_after[k], engine_before[k])
