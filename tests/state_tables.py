"""Hand-built states for the expand and snapshot tests, on the CPU: wall_table() is the local transition table of tests/test_expand.py with the agent's
cell as a parameter (every wall and corner, grids of up to 255 x 255), painted_states() the small fixed batch of state classes a painter can get wrong,
oracle_frame() the oracle's rasterisers for one state.  Numpy arrays in and out, no GPU.  A plain module, not a fixture; tests/test_state_tables_logic.py
counts from the oracle alone what the tables exercise."""
import ctypes as C
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


# ------------------------------------------------------------------------------------------------------------------------------ the table at any wall
def _parking(S, ar, ac):
    """-> the cells of the init grid's eight objects around an agent at (ar, ac): [sticks, axe, hammer, tree], [rock, bread, house, wheat] -- two rows at row
    distance 2 and 3 from the anchor on the side that exists (below it if there is room), in each the four columns of the half farther from the anchor's"""
    down = ar + 3 < S
    rows = (ar + 2, ar + 3) if down else (ar - 2, ar - 3)
    cols = list(range(S - 4, S)) if ac < S // 2 else list(range(4))
    return [(rows[0], c) for c in cols], [(rows[1], c) for c in cols]


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
    if span == 'full':
        per = [c for c in product(range(9), UNDER, range(4), range(4), range(4), range(3)) if not (c[0] and c[0] == c[1])]
    else:
        per = []
        for i, (tgt, hold, side) in enumerate(product(range(9), range(4), range(4))):
            under = UNDER[i % 6]                             # (the three cycles shifted against each other: periods 6, 4 and 3 alone repeat every 12 cases)
            per.append((tgt, 0 if under == tgt else under, hold, side, (i + i // 16) % 4, (i // 7) % 3))
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
