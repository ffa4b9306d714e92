"""The fixed call sequences of tests/test_call_sequences.py -- pure numpy, TEST INFRASTRUCTURE ONLY.  A script is an Eulerian circuit of the complete
directed graph over MUTATORS (loops included), so every ordered pair of state-changing calls occurs once with nothing between its two calls (gap = 0)
or with `gap` steps between them; after every K-th op the batch takes a segment of max_steps + 2 steps (look-ahead rings drain and refill), and the
script ends with 2 * max_steps + 3 steps.  A checkpoint is loaded two mutators after it was saved, as an op of its own ('ckpt_load').  That load and the
step segments fall BETWEEN the two calls of some pair: the pairs they break are played again behind the circuit, until every ordered pair occurs with
nothing (or exactly the gap) between its calls.  Masks, desired bits, bank rows, phases and actions
come from one seeded RandomState: a script is a function of build()'s arguments and nothing else.  tests/test_sequence_script_logic.py checks the
conditions a script has to meet, from the CPU model alone."""
import numpy as np

MUTATORS = ('reset', 'reset_envs', 'imagine', 'imagine_commit', 'sample', 'save', 'load_stream', 'load_episode', 'set_phase', 'set_rng', 'ckpt_save')
CKPT_LOAD_AFTER = 2                                  # a checkpoint is loaded this many ops after its save
CAP = 96                                             # rows of the bank
NEVER = (90, 96)                                     # rows no save ever names: [90, 96)
PAST = (CAP, CAP + 5)                                # rows past the bank a load names
K_OPS = 6                                            # a step segment follows every K_OPS-th op
BASE = 77000                                         # env i starts from numpy's RandomState(BASE + i)
SEEDS = {0: 18, 2: 1}                                # gap -> the script's seed (tests/test_sequence_script_logic.py: the conditions hold for these)
KINDS = ('state_manual', 'dirty_ray_auto', 'pixels_alt_auto', 'state_auto_pool_menus', 'pixels_ray_auto')
RUNS = [(kind, 5, gap) for kind in KINDS for gap in (0, 2)] + [('pixels_ray_auto', 8, 0)]      # 8 x 8: the full-frame engine's other painter
N_VARIANTS = 1000                                    # a step segment carries a number below this; the driver maps it onto the step variants its engine has


def circuit(n, rs):
    """an Eulerian circuit of the complete directed graph on n nodes with loops, from node 0 (Hierholzer, the edges of a node in an order drawn from
    rs) -> n * n + 1 nodes, the last one node 0 again"""
    out_edges = [list(rs.permutation(n)) for _ in range(n)]
    stack, tour = [0], []
    while stack:
        v = stack[-1]
        if out_edges[v]:
            stack.append(int(out_edges[v].pop()))
        else:
            tour.append(stack.pop())
    return tour[::-1]


def layout(seq, K, gap):
    """the mutator sequence with everything that falls between its calls -> tokens: a mutator's number, 'load' (a checkpoint is loaded CKPT_LOAD_AFTER
    mutators after its save, as an op of its own; those still due at the end follow the last mutator), 'segment' (after every K-th op, loads
    included) and 'gap' (after every other op, if gap > 0)"""
    ck = MUTATORS.index('ckpt_save')
    out, count, due = [], 0, []

    def op(tok):
        nonlocal count
        out.append(tok)
        count += 1
        if count % K == 0:
            out.append('segment')
        elif gap:
            out.append('gap')

    for m in seq:
        op(int(m))
        due = [d - 1 for d in due] + ([CKPT_LOAD_AFTER] if m == ck else [])
        while due and due[0] <= 0:
            due.pop(0)
            op('load')
    for _ in due:
        op('load')
    return out


def unbroken_pairs(tokens, gap):
    """the ordered pairs (a, b) of mutators that occur with nothing between a and b -- or, in a script with a gap, with exactly the gap's steps"""
    at = [i for i, t in enumerate(tokens) if isinstance(t, int)]
    between = ['gap'] if gap else []
    return {(tokens[i], tokens[j]) for i, j in zip(at, at[1:]) if tokens[i + 1:j] == between}


def mutator_sequence(rs, K, gap):
    """the circuit, then -- again and again -- the pairs a checkpoint load or a step segment fell between, until every ordered pair occurs unbroken"""
    n = len(MUTATORS)
    seq = circuit(n, rs)
    every = {(a, b) for a in range(n) for b in range(n)}
    for _ in range(40):
        missing = sorted(every - unbroken_pairs(layout(seq, K, gap), gap))
        if not missing:
            return seq
        for k in rs.permutation(len(missing)):
            seq += list(missing[k])
    raise AssertionError('no sequence with every pair unbroken')


def _mask(rs, N):
    """at least a quarter of the envs selected, at least a quarter left"""
    k = int(rs.randint((N + 3) // 4, N - (N + 3) // 4 + 1))
    m = np.zeros(N, np.uint8)
    m[rs.permutation(N)[:k]] = 1
    return m


def _save_rows(rs, N):
    """two envs in three into distinct rows below NEVER[0], one env into a row past the bank (skipped and counted), the rest take no part"""
    rows = np.full(N, -1, np.int32)
    envs = rs.permutation(N)
    k = 2 * N // 3
    rows[envs[:k]] = rs.permutation(NEVER[0])[:k]
    rows[envs[k]] = PAST[0] + int(rs.randint(PAST[1] - PAST[0]))
    return rows


def _load_rows(rs, N, saved):
    """a fork (a seventh of the envs from one saved row), saved rows in a drawn order over half of the envs, and among the rest -1, a row past the bank
    and a never-saved row; before the first save every row named is a never-saved one"""
    rows = np.full(N, -1, np.int32)
    envs = rs.permutation(N)
    fork, perm = N // 7, N // 2
    if saved:
        s = np.array(sorted(saved), np.int32)
        rows[envs[:fork]] = s[rs.randint(len(s))]
        rows[envs[fork:fork + perm]] = s[rs.permutation(len(s))[np.arange(perm) % len(s)]]
    else:
        rows[envs[:fork + perm]] = rs.randint(NEVER[0], NEVER[1], fork + perm)
    rows[envs[fork + perm]] = PAST[0] + int(rs.randint(PAST[1] - PAST[0]))
    rows[envs[fork + perm + 1]] = int(rs.randint(NEVER[0], NEVER[1]))
    rows[envs[fork + perm + 2]] = -7
    return rows


def build(seed, N, max_steps, gap=0, K=K_OPS, pooled=False):
    """-> the script: a list of (name, args) -- the MUTATORS, 'ckpt_load' and 'steps' (args: actions uint8 [T, N], variant)"""
    rs = np.random.RandomState(seed)
    ops, saved = [], set()
    for tok in layout(mutator_sequence(rs, K, gap), K, gap):
        name = MUTATORS[tok] if isinstance(tok, int) else tok
        args = {}
        if name in ('segment', 'gap'):
            T = max_steps + 2 if name == 'segment' else gap
            name, args = 'steps', dict(actions=rs.randint(0, 6, (T, N)).astype(np.uint8), variant=int(rs.randint(N_VARIANTS)))
        elif name == 'load':
            name = 'ckpt_load'
        elif name == 'reset_envs':
            args = dict(mask=_mask(rs, N))
        elif name in ('imagine', 'imagine_commit'):
            args = dict(mask=_mask(rs, N), desired=rs.randint(0, 512, N).astype(np.uint16))
        elif name == 'sample':
            args = dict(mask=_mask(rs, N), pooled=bool(pooled))
        elif name == 'save':
            rows = _save_rows(rs, N)
            saved |= set(rows[(rows >= 0) & (rows < CAP)].tolist())
            args = dict(rows=rows)
        elif name in ('load_stream', 'load_episode'):
            args = dict(rows=_load_rows(rs, N, saved))
        elif name == 'set_phase':
            args = dict(phases=rs.randint(0, max_steps, N).astype(np.int32))
        elif name == 'set_rng':
            args = dict(base=int(rs.randint(1, 2 ** 20)))
        ops.append((name, args))
    ops.append(('steps', dict(actions=rs.randint(0, 6, (2 * max_steps + 3, N)).astype(np.uint8), variant=int(rs.randint(N_VARIANTS)))))
    return ops


def rng_states(N, base):
    """the streams a 'set_rng' op injects: numpy's RandomState(base + i) after 1, 624 or 625 + i draws -- early in a generation, at its very end
    (position 624) and anywhere in the next one.  Every key is one a twist produced: of a key straight from a seed the low 31 bits of word 0 are not
    part of the generator's state, and an engine need not hand them back."""
    keys, pos = np.empty((N, 624), np.uint32), np.empty(N, np.int32)
    for i in range(N):
        rs = np.random.RandomState(base + i)
        rs.randint(0, 2 ** 32, (1, 624, 625 + i)[i % 3], dtype=np.uint32)
        st = rs.get_state()
        keys[i], pos[i] = st[1], st[2]
    return keys, pos


def script_of(kind, gap):
    """the script of one of RUNS (the grid's size does not enter)"""
    from engines import K5, N1
    return build(SEEDS[gap], N1, K5['max_steps'], gap, pooled=kind == 'state_auto_pool_menus')


def tokens_of(ops, max_steps):
    """a script back as layout()'s tokens (the closing steps left out), for the pair condition"""
    out = []
    for name, args in ops[:-1]:
        if name == 'steps':
            out.append('segment' if len(args['actions']) == max_steps + 2 else 'gap')
        else:
            out.append('load' if name == 'ckpt_load' else MUTATORS.index(name))
    return out


def describe(ops, i):
    """op i and the three ops before it, for a failure message"""
    return ' <- '.join('%d:%s' % (j, ops[j][0] + ('[%d]' % len(ops[j][1]['actions']) if ops[j][0] == 'steps' else '')) for j in range(i, max(i - 4, -1), -1))


def failure(kind, size, gap, ops, i, how, err):
    """the message of a comparison that failed after op i: the run, the op, the three ops before it, how a step segment ran, and what differed"""
    return '%s %dx%d, gap %d, seed %d: after op %s%s: %s' % (kind, size, size, gap, SEEDS[gap], describe(ops, i), ' (%s)' % how if how else '', err)
