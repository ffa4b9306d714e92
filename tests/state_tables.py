"""Hand-built states for the expand and snapshot tests, on the CPU: local_table() is the local transition table of tests/test_expand.py, wall_table() the
same with the agent's cell as a parameter (every wall and corner, grids of up to 255 x 255), painted_states() the small fixed batch of state classes a
painter can get wrong, oracle_frame() the oracle's rasterisers for one state.  load_table_fixture() reads what the REFERENCE classes answered on two of
these tables (tests/golden/table5_ray.npz, walls8_ray_alt.npz; written by tools/gen_table_golden.py) and first_difference() / same_table() compare such
columns row by row.  Numpy arrays in and out, no GPU.  A plain module, not a fixture; tests/test_state_tables_logic.py counts from the oracle alone what
the tables exercise, tests/test_table_golden_logic.py from the reference's rows alone."""
import ctypes as C
import functools
import json
import os
import zlib
from itertools import product

import numpy as np

DR = [(-1, 0), (0, 1), (1, 0), (0, -1)]                     # up, right, down, left (ray.py:130-131)
UNDER, ACH = (0, 1, 2, 3, 7, 8), (0, 1 << 3, 0x1FF)          # what lies under the agent; the achieved word a case starts from
MIN_S = 8                                                   # below it the parked objects could touch the agent's neighbours
LARGE_S, LARGE_CAP = 182, 512                               # from this size on a table is capped: oracle_successors holds 6 M S^2 bytes of grids


def oracle_frame(grid, agent, hold, alt):
    """the oracle's full-frame rasteriser of one state (ray.py:442-520, alt: craftingworld_altobs.py:489-560 modulo 256) -> uint8 [4S, 4S, 3] or
    [3S + 3, 3S, 3]"""
    from oracle.oracle import _lib
    lib, u8p = _lib(), C.POINTER(C.c_uint8)
    g = np.ascontiguousarray(grid, dtype=np.uint8)
    s = g.shape[0]
    out = np.empty((3 * s + 3, 3 * s, 3) if alt else (4 * s, 4 * s, 3), dtype=np.uint8)
    fn = lib.cwo_render_alt if alt else lib.cwo_render
    fn.argtypes = [C.c_int32, u8p, C.c_int32, C.c_int32, C.c_int32, u8p]
    fn.restype = None
    fn(s, g.ctypes.data_as(u8p), int(agent[0]), int(agent[1]), int(hold), out.ctypes.data_as(u8p))
    return out


# ------------------------------------------------------------------------------------------------------------------------------ the local table
LOCAL_S, LOCAL_MAX_STEPS = 5, 9


def local_cases():
    """the case tuples of local_table(), in its order: (object in the target cell, object under the agent, hold, side, initv, achv, wall)"""
    return [c for c in product(range(9), UNDER, range(4), range(4), range(4), range(3), (0, 1)) if not (c[0] and c[0] == c[1])]


@functools.lru_cache(maxsize=None)
def local_table():
    """The states of test_hip_parity.test_systematic_transition_table without its action dimension: (object in the target cell 0..8) x (object under the
    agent) x (hold) x (the side 0..3 on which the target cell lies) x (where the init grid put sticks / axe / hammer / tree relative to the two cells) x
    (achieved bits) x (agent interior / in the corner); target and under never the same non-empty code.  -> grid, init_grid [n, 5, 5], agent [n, 2], hold,
    achieved [n]"""
    S = LOCAL_S
    cases = []
    for tgt, under, hold, side, initv, achv, wall in local_cases():
        ar, ac = (0, 0) if wall else (2, 2)
        g = np.zeros((S, S), np.uint8)
        g[ar, ac] = under
        tr, tc = ar + DR[side][0], ac + DR[side][1]
        if 0 <= tr < S and 0 <= tc < S:
            g[tr, tc] = tgt
        else:
            tr, tc = ar, ac                      # the wall: target == own cell
        ig = np.zeros((S, S), np.uint8)          # one of each object; objects 1, 2, 3, 5 placed per initv
        spots = {0: [(4, 0), (4, 1), (4, 2), (4, 3)],
                 1: [(tr, tc), (4, 1), (4, 2), (4, 3)],
                 2: [(4, 0), (tr, tc), (4, 2), (4, 3)] if hold != 3 else [(4, 0), (4, 1), (tr, tc), (4, 3)],
                 3: [(4, 0), (4, 1), (4, 2), (tr, tc)]}[initv]
        for code, (r, c) in zip((1, 2, 3, 5), spots):
            ig[r, c] = code
        for code, (r, c) in zip((4, 6, 7, 8), [(3, 4), (2, 4), (1, 4), (0, 4)]):
            ig[r, c] = code
        cases.append((g, ig, (ar, ac), hold, ACH[achv]))
    assert len(cases) == 18816
    return (np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases]), np.array([c[2] for c in cases], np.int64),
            np.array([c[3] for c in cases], np.int64), np.array([c[4] for c in cases], np.int64))


# ------------------------------------------------------------------------------------------------------------------------------ the table at any wall
def _parking(S, ar, ac):
    """-> the cells of the init grid's eight objects around an agent at (ar, ac): [sticks, axe, hammer, tree], [rock, bread, house, wheat] -- two rows at row
    distance 2 and 3 from the anchor on the side that exists (below it if there is room), in each the four columns of the half farther from the anchor's"""
    down = ar + 3 < S
    rows = (ar + 2, ar + 3) if down else (ar - 2, ar - 3)
    cols = list(range(S - 4, S)) if ac < S // 2 else list(range(4))
    return [(rows[0], c) for c in cols], [(rows[1], c) for c in cols]


def _span_cases(span):
    """the case tuples of one anchor of wall_table(): (object in the target cell, object under the agent, hold, side, initv, achv)"""
    if span == 'full':
        return [c for c in product(range(9), UNDER, range(4), range(4), range(4), range(3)) if not (c[0] and c[0] == c[1])]
    per = []
    for i, (tgt, hold, side) in enumerate(product(range(9), range(4), range(4))):
        under = UNDER[i % 6]                                 # (the three cycles shifted against each other: periods 6, 4 and 3 alone repeat every 12 cases)
        per.append((tgt, 0 if under == tgt else under, hold, side, (i + i // 16) % 4, (i // 7) % 3))
    return per


def wall_cases(anchors, span='reduced'):
    """the case tuples of wall_table(S, anchors, ..., span), in its order: (anchor, object in the target cell, object under the agent, hold, side, initv, achv)"""
    return [((int(r), int(c)),) + tuple(case) for r, c in anchors for case in _span_cases(span)]


def wall_table(S, anchors, max_states, span='reduced'):
    """test_expand._table() with the agent's cell as a parameter: for each anchor (ar, ac) the states (object in the target cell 0..8) x (hold 0..3) x (the
    side 0..3 on which the target cell lies), target and under never the same non-empty code; a side that leaves the grid makes the target the agent's own
    cell.  span='reduced' (144 states an anchor): what lies under the agent, where the init grid put sticks / axe / hammer / tree relative to the two cells
    and the achieved word cycle with the case index; span='full' (9 408 an anchor): every combination of them, as _table() has.  The init grid holds one
    of each object, parked (_parking) clear of the anchor and its four neighbours; sticks, axe, hammer or tree moves onto the target cell per initv.
    -> grid, init_grid uint8 [n, S, S], agent [n, 2], hold, achieved [n].  ValueError above max_states states, for S < 8, an anchor off the grid, an
    unknown span, and from S = 182 on above 512 states whatever max_states says."""
    if S < MIN_S:
        raise ValueError('wall_table needs S >= %d, got %d' % (MIN_S, S))
    if span not in ('reduced', 'full'):
        raise ValueError('span must be reduced or full, got %r' % (span,))
    anchors = [(int(r), int(c)) for r, c in anchors]
    if not anchors or any(not (0 <= r < S and 0 <= c < S) for r, c in anchors):
        raise ValueError('anchors must be cells of the %d x %d grid' % (S, S))
    per = _span_cases(span)
    n = len(per) * len(anchors)
    cap = min(int(max_states), LARGE_CAP) if S >= LARGE_S else int(max_states)
    if n > cap:
        raise ValueError('%d states at S = %d, at most %d' % (n, S, cap))
    grid, init = np.zeros((n, S, S), np.uint8), np.zeros((n, S, S), np.uint8)
    agent, hold_a, ach = np.zeros((n, 2), np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    j = 0
    for ar, ac in anchors:
        movable, fixed = _parking(S, ar, ac)
        for tgt, under, hold, side, initv, achv in per:
            grid[j, ar, ac] = under
            tr, tc = ar + DR[side][0], ac + DR[side][1]
            if 0 <= tr < S and 0 <= tc < S:
                grid[j, tr, tc] = tgt
            else:
                tr, tc = ar, ac                              # the wall: target == own cell
            spots = list(movable)
            if initv:
                spots[{1: 0, 2: 1 if hold != 3 else 2, 3: 3}[initv]] = (tr, tc)
            for code, (r, c) in zip((1, 2, 3, 5), spots):
                init[j, r, c] = code
            for code, (r, c) in zip((4, 6, 7, 8), fixed):
                init[j, r, c] = code
            agent[j], hold_a[j], ach[j] = (ar, ac), hold, ACH[achv]
            j += 1
    assert j == n and ((init != 0).sum(axis=(1, 2)) == 8).all()
    return grid, init, agent, hold_a, ach


def table_desired(table, oracle_kw, seed=1):
    """desired of state i: for about half of the states (RandomState(seed)) the achieved mask the oracle gets for action i % 6 -- a goal one step away --
    else randint(1, 512).  The oracle runs over that half only."""
    from expand_check import oracle_successors
    grid, init, agent, hold, ach = table
    n = len(hold)
    rng = np.random.RandomState(seed)
    near = np.flatnonzero(rng.rand(n) < 0.5)
    des = rng.randint(1, 512, n).astype(np.int64)
    z = np.zeros(len(near), np.int64)
    suc = oracle_successors(dict(grid=grid[near], agent=agent[near], hold=hold[near], achieved=ach[near], desired=z + 1, step_num=z + 3, flags=z), init[near],
                            oracle_kw)
    des[near] = suc['achieved'][near % 6, np.arange(len(near))]
    return des


def table_coverage(states, suc):
    """what a table exercises, counted from the oracle's successors alone -> dict: gains [9] and losses [4] (bits 5..8) of task bits over all rows, changed /
    unchanged rows, unchanged rows of each of the four moves, changed pickups and drops"""
    ach = np.asarray(states['achieved']).astype(np.int64)
    gained, lost = suc['achieved'] & ~ach, ach & ~suc['achieved']
    return dict(gains=[int(((gained >> b) & 1).sum()) for b in range(9)], losses=[int(((lost >> b) & 1).sum()) for b in range(5, 9)],
                changed=int(suc['changed'].sum()), unchanged=int((~suc['changed']).sum()), blocked_moves=[int((~suc['changed'][a]).sum()) for a in range(4)],
                pickups=int(suc['changed'][4].sum()), drops=int(suc['changed'][5].sum()))


# ------------------------------------------------------------------------------------------------------------------------------ the state classes of a painter
def _base_cells(S):
    """cells of objects 1..8 in the start state of every painted state: spread over the whole grid (at S = 255 most lie above 32 767), none in a corner or
    beside one"""
    nc = S * S
    keep_free = {0, 1, 2, S - 2, S - 1, S, nc - S - 1, nc - S, nc - S + 1, nc - 2, nc - 1, 2 * S - 1, S * (S - 2)}
    stride, cells = (nc - 3) // 8, []
    for k in range(7):
        c = 3 + k * stride
        while c in keep_free or c in cells:
            c += 1
        cells.append(c)
    cells.append(nc - S - 3)                                # the wheat in the last row but one: above 32 767 from 182 x 182 on
    assert len(set(cells)) == 8 and max(cells) < nc
    return cells


def painted_states(S):
    """A small fixed batch of states for the tests of a painting load -> list of (name, grid uint8 [S, S], init_grid uint8 [S, S], agent (r, c), hold).  The
    init grid holds one of each object; a held item is off the grid, so no state has more than eight objects.  Every state is reachable: objects 1-3 move
    by being carried, a tree leaves sticks, sticks under the hammer a house, wheat under the axe bread, rock and bread vanish."""
    if S < 5:
        raise ValueError('painted_states needs S >= 5')
    nc = S * S
    cells = _base_cells(S)
    init = np.zeros(nc, np.uint8)
    for k, c in enumerate(cells):
        init[c] = k + 1
    at = {k + 1: (c // S, c % S) for k, c in enumerate(cells)}                    # code -> its start cell
    free = next(c for c in range(3, nc) if init[c] == 0 and c not in (S - 1, S * (S - 1), nc - 1))
    out = []

    def add(name, agent, hold, edit=(), init_edit=()):
        g, ig = init.copy(), init.copy()
        if hold:
            g[cells[hold - 1]] = 0                                                 # the held item left its cell
        for c, code in edit:
            g[c] = code
        for c, code in init_edit:
            ig[c] = code
        assert (g != 0).sum() + (hold != 0) <= 8 and all((ig == k).sum() <= 1 for k in range(1, 9))
        out.append((name, g.reshape(S, S), ig.reshape(S, S), (int(agent[0]), int(agent[1])), int(hold)))

    for h in range(4):
        add('hold %d on an empty cell' % h, (free // S, free % S), h)
    for h, under in ((0, 8), (1, 3), (2, 1), (3, 2)):
        add('hold %d standing on object %d' % (h, under), at[under], h)
    add('sticks held over a sticks cell', at[5], 1, edit=[(cells[4], 1)])          # the chopped tree's sticks under the carried ones
    add('axe held on the wheat-turned-bread cell', at[8], 2, edit=[(cells[7], 6)])
    add('a house under the agent', at[7], 0)
    add('rock and bread both gone', at[4], 0, edit=[(cells[3], 0), (cells[5], 0)])
    for k, (r, c) in enumerate([(0, 0), (0, S - 1), (S - 1, 0), (S - 1, S - 1)]):
        add('corner (%d, %d) holding nothing' % (r, c), (r, c), 0)
        add('corner (%d, %d) holding %d' % (r, c, 1 + k % 3), (r, c), 1 + k % 3)
    add('an object in cell 0', (0, 1), 0, edit=[(cells[1], 0), (0, 2)], init_edit=[(cells[1], 0), (0, 2)])
    add('an object in cell S*S - 1', (S - 1, S - 2), 1, edit=[(cells[2], 0), (nc - 1, 3)], init_edit=[(cells[2], 0), (nc - 1, 3)])
    return out


def painted_batch(S, N):
    """painted_states(S) tiled over N envs -> (names [N], grid [N, S, S], init_grid [N, S, S], agent uint8 [N, 2], hold uint8 [N])"""
    ps = painted_states(S)
    pick = [ps[i % len(ps)] for i in range(N)]
    return ([p[0] for p in pick], np.stack([p[1] for p in pick]), np.stack([p[2] for p in pick]), np.array([p[3] for p in pick], np.uint8),
            np.array([p[4] for p in pick], np.uint8))


# ------------------------------------------------------------------------------------------------------------------------------ what the reference answered on a table
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
WALLS8_ANCHORS = [(0, 0), (0, 7), (7, 0), (7, 7), (0, 4), (4, 7), (7, 4), (4, 0), (3, 3)]     # the four corners, the four mid-edge cells, one interior cell
TABLE_FIXTURES = {'table5_ray': dict(table='local_table()', S=LOCAL_S, max_steps=LOCAL_MAX_STEPS, step_nums=[3, LOCAL_MAX_STEPS - 1]),
                  'walls8_ray_alt': dict(table="wall_table(8, WALLS8_ANCHORS, 1296, span='reduced')", S=8, max_steps=LOCAL_MAX_STEPS, step_nums=[3])}
INPUTS = (('grid', np.uint8), ('init_grid', np.uint8), ('agent', np.uint8), ('hold', np.uint8), ('achieved0', np.uint16))
DYNAMICS = ('achieved', 'agent', 'hold', 'own', 'new')       # per (action, state): what the state becomes; own / new: the codes left in the start cell and in the end cell
OUTCOME = ('reward', 'done')                                 # per (reward rule: equal, subset; step_num; action; state)


def _crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF


def fixture_table(name):
    """the states a table fixture was recorded on, rebuilt -> ((grid, init_grid, agent, hold, achieved), the case tuple of every state)"""
    if name == 'table5_ray':
        return local_table(), local_cases()
    if name == 'walls8_ray_alt':
        return wall_table(8, WALLS8_ANCHORS, 1296, span='reduced'), wall_cases(WALLS8_ANCHORS, 'reduced')
    raise ValueError('no table fixture %r' % (name,))


def input_crcs(table):
    """CRC32 of each input array of a table in the dtype INPUTS names -- what a fixture's meta pins"""
    return {k: _crc(np.asarray(a).astype(dt)) for (k, dt), a in zip(INPUTS, table)}


def successor_grids(grid, agent, agent_after, own, new):
    """the six successor grids of every state from the two codes a step can change: the state's grid, then the start cell = own, then the end cell = new
    (in that order: a blocked move ends on the start cell) -> uint8 [6, n, S, S]"""
    n = len(grid)
    j = np.arange(n)
    out = np.repeat(np.asarray(grid, np.uint8)[None], 6, axis=0)
    for a in range(6):
        out[a, j, agent[:, 0], agent[:, 1]] = own[a]
        out[a, j, agent_after[a, :, 0], agent_after[a, :, 1]] = new[a]
    return out


def load_table_fixture(name, path=None):
    """tests/golden/<name>.npz: the reference's answers on the table fixture_table(name) rebuilds.  The inputs are checked against the CRCs in meta.
    -> dict: meta, table, cases, n, S, max_steps, step_nums, the stored columns (desired [n]; achieved, hold, own, new [6, n]; agent [6, n, 2]; reward,
    done [2, len(step_nums), 6, n]; walls8_ray_alt: crc_ray, crc_alt [6, n]) as int64 and grid uint8 [6, n, S, S], the successor grids"""
    table, cases = fixture_table(name)
    z = np.load(path or os.path.join(GOLDEN, name + '.npz'))
    d = {k: z[k] for k in z.files}
    meta = json.loads(bytes(d.pop('meta')).decode())
    if meta['name'] != name or (meta['S'], meta['max_steps'], meta['step_nums']) != tuple(TABLE_FIXTURES[name][k] for k in ('S', 'max_steps', 'step_nums')):
        raise ValueError('%s: meta %r does not describe this table' % (name, meta))
    crcs = input_crcs(table)
    if meta['input_crc'] != crcs:
        raise ValueError('%s: the table rebuilt here is not the one the fixture was recorded on: CRCs %r, recorded %r' % (name, crcs, meta['input_crc']))
    n = len(cases)
    out = dict(meta=meta, table=table, cases=cases, n=n, S=meta['S'], max_steps=meta['max_steps'], step_nums=meta['step_nums'])
    for k, v in d.items():
        out[k] = v.astype(np.int64)
    if 'crc_index' in out:                                   # (frames stored once per distinct successor)
        for k in ('crc_ray', 'crc_alt'):
            out[k] = out[k][out['crc_index']]
        del out['crc_index']
    shapes = dict(desired=(n,), achieved=(6, n), agent=(6, n, 2), hold=(6, n), own=(6, n), new=(6, n), reward=(2, len(meta['step_nums']), 6, n),
                  done=(2, len(meta['step_nums']), 6, n))
    for k, shape in shapes.items():
        if out[k].shape != shape:
            raise ValueError('%s: %s has shape %s, expected %s' % (name, k, out[k].shape, shape))
    out['grid'] = successor_grids(table[0], table[2], out['agent'], out['own'], out['new'])
    return out


def first_difference(field, want, got, cases):
    """-> None where the arrays are equal, else (state index, action or None, field, the table's case tuple of that state, got, expected) of the first
    differing row in C order.  The state axis is the one as long as `cases`, the action the axis before it (none: a per-state column)."""
    want, got = np.asarray(want), np.asarray(got)
    if want.shape != got.shape:
        raise ValueError('%s: shapes %s and %s' % (field, got.shape, want.shape))
    axis = [i for i, m in enumerate(want.shape) if m == len(cases)]
    if not axis:
        raise ValueError('%s: no axis of shape %s holds the %d states' % (field, want.shape, len(cases)))
    bad = np.argwhere(want != got)
    if len(bad) == 0:
        return None
    i = tuple(int(x) for x in bad[0])
    state = i[axis[0]]
    return state, (i[axis[0] - 1] if axis[0] else None), field, cases[state], got[i].item(), want[i].item()


def same_table(want, got, cases, fields=None, tag=''):
    """every field of `fields` (default: all of want's) equal in want and got, or an AssertionError naming the first differing row: state index, action,
    field, the table's case tuple"""
    for f in fields or sorted(want):
        d = first_difference(f, want[f], got[f], cases)
        assert d is None, '%s%s differs first at state %d, action %s: got %r, expected %r; the table\'s case %r' % (tag, d[2], d[0], d[1], d[4], d[5], d[3])
