"""What "cw_load_records did exactly what it should" means, in one place -- pure numpy, no GPU.  record_rule() is the rule an env applies to a record before
it takes it, written here a second time from the text of include/craftingworld.h (tests/test_load_records_host.py holds the library's cwh_record_ok against
it); MUTATIONS are the single defects of a good record that the rule must refuse; walk_records() are the records of oracle random walks, which it must
accept; check_load_records() compares masked_check.take() snapshots taken around a load with the contract: EVERY loaded env against its record -- header
but the menu byte, slots, the dense state, the mask outputs and, in the pixel modes, the observation frame by the oracle's rasteriser --, everything else
of a loaded env and every other env byte for byte against the before-snapshot, counters[6] against the skipped and refused envs, and the status bytes.
A plain module, not a fixture; tests/test_load_records_logic.py tests the comparison itself with deliberately wrong snapshots."""
import numpy as np

from oracle_replay import same
from records_check import POS_GONE, POS_HELD, decode, encode
from state_tables import oracle_frame

SKIPPED = 6                                                 # counters[6]: envs a snapshot or record load skipped
NO_PART, LOADED, BAD_INDEX, REFUSED = range(4)              # the status bytes
WALK_SIZES, WALK_ENVS, WALK_STEPS = (4, 5, 8), 12, 400      # the oracle walks every record of which an env must take


def record_rule(S, hdr, slot_pos):
    """the rule of cw_load_records for one record (hdr uint8 [16], slot_pos uint16 [8]) on an S x S grid -> bool"""
    hdr = np.asarray(hdr, dtype=np.uint8).reshape(16).astype(np.int64)
    pos = np.ascontiguousarray(slot_pos).reshape(8).view(np.uint16).astype(np.int64)
    hold = int(hdr[2])
    if not (hdr[0] < S and hdr[1] < S and hold <= 3):
        return False
    codes = [int(hdr[12 + k // 2] >> (4 * (k % 2))) & 15 for k in range(8)]
    on_grid, held = [], 0
    for k in range(8):
        p, c = int(pos[k]), codes[k]
        if c > 8:
            return False
        if p == POS_GONE:
            if c != 0:
                return False
        elif p == POS_HELD:
            if hold == 0 or c != hold:
                return False
            held += 1
        elif p < S * S:
            if c == 0:
                return False
            on_grid.append(p)
        else:
            return False
    return held == (1 if hold else 0) and len(set(on_grid)) == len(on_grid)


def good_record(S, last_cell=False):
    """a record every env of size S >= 4 takes: the axe held, one slot gone, six objects on the grid -- one of them in cell S * S - 1 if last_cell --, flags
    and masks set -> (hdr uint8 [16], slot_pos uint16 [8])"""
    hdr = np.zeros(16, np.uint8)
    hdr[0:4] = (1, 2, 2, 0)
    hdr[4:12] = (0x08, 0x00, 0x49, 0x01, 3, 0, 2, 0)        # achieved, desired, step_num 3, the subset flag
    cells = [0, POS_HELD, S * S - 1 if last_cell else 6, 5, POS_GONE, 7, 8, 9]
    codes = [1, 2, 3, 4, 0, 6, 7, 8]
    for k, c in enumerate(codes):
        hdr[12 + k // 2] |= c << (4 * (k % 2))
    return hdr, np.array(cells, np.uint16)


def _set_code(hdr, k, code):
    hdr[12 + k // 2] = (int(hdr[12 + k // 2]) & (0xF0 if k % 2 == 0 else 0x0F)) | (code << (4 * (k % 2)))


def _mut(name, S, hdr, pos):
    """one single mutation of good_record(S), in place (slot 1 is held with code 2, slot 4 gone, the others on the grid)"""
    if name.startswith('agent'):
        hdr[0 if 'row' in name else 1] = S if name.endswith('= S') else 255
    elif name == 'hold 4':
        hdr[2] = 4
    elif name.startswith('code '):
        _set_code(hdr, 3, int(name.split()[1]))
    elif name == 'position S*S':
        pos[3] = S * S
    elif name == 'position 0xFFFD':
        pos[3] = 0xFFFD
    elif name == 'gone with a code':
        _set_code(hdr, 4, 5)
    elif name == 'on-grid with code 0':
        _set_code(hdr, 3, 0)
    elif name == 'held without hold':
        hdr[2] = 0
    elif name == 'hold without held':
        pos[1] = POS_GONE
        _set_code(hdr, 1, 0)
    elif name == 'two held':
        pos[0] = POS_HELD
        _set_code(hdr, 0, 2)
    elif name == 'held code != hold':
        _set_code(hdr, 1, 3)
    elif name == 'two on-grid slots on one cell':
        pos[5] = pos[3]
    else:
        raise ValueError(name)


MUTATIONS = ('agent row = S', 'agent col = S', 'agent row = 255', 'agent col = 255', 'hold 4', 'code 9', 'code 15', 'position S*S', 'position 0xFFFD',
             'gone with a code', 'on-grid with code 0', 'held without hold', 'hold without held', 'two held', 'held code != hold',
             'two on-grid slots on one cell')


def mutated(name, S):
    """good_record(S) with the single mutation `name` of MUTATIONS"""
    hdr, pos = good_record(S)
    _mut(name, S, hdr, pos)
    return hdr, pos


def dense_of(envs, flags=0):
    """oracle envs as the dense states records_check.encode takes"""
    from oracle_replay import oracle_arrays
    a = oracle_arrays(envs, [])
    return dict(grid=a['grid'], agent=a['agent_rc'], hold=a['hold'], achieved=a['achieved'], desired=a['desired'], step_num=a['step_num'],
                flags=np.full(len(envs), flags, np.int64))


def walk_records(S, n_envs=WALK_ENVS, steps=WALK_STEPS, seed=0):
    """the records of an oracle random walk: n_envs envs of size S, max_steps 17, auto-reset, `steps` uniform actions each, encoded after every step ->
    (hdr uint8 [steps * n_envs, 16], slot_pos uint16 [steps * n_envs, 8])"""
    from oracle import OracleBatch
    from oracle_replay import np_states
    keys, pos = np_states(n_envs, 9000 + 100 * S + seed)
    ora = OracleBatch(n_envs, rng_states=list(zip(keys, pos)), size=(S, S), max_steps=17)
    ora.reset()
    acts = np.random.RandomState(seed + S).randint(0, 6, (steps, n_envs))
    hs, ps = [], []
    for t in range(steps):
        ora.step(acts[t])
        h, p = encode(dense_of(ora.envs))
        hs.append(h)
        ps.append(p)
    return np.concatenate(hs), np.concatenate(ps)


def expected_status(N, R, S, hdr, slot_pos, src):
    """-> the status byte of every env: src None is record i for env i (R must be N)"""
    if src is None:
        if R != N:
            raise ValueError('%d records for %d envs without src' % (R, N))
        src = np.arange(N)
    src = np.asarray(src).reshape(-1).astype(np.int64)
    if len(src) != N:
        raise ValueError('%d src entries for %d envs' % (len(src), N))
    out = np.zeros(N, np.uint8)
    verdict = {}
    for i, j in enumerate(src.tolist()):
        if j < 0:
            continue
        if j >= R:
            out[i] = BAD_INDEX
            continue
        if j not in verdict:
            verdict[j] = record_rule(S, hdr[j], slot_pos[j])
        out[i] = LOADED if verdict[j] else REFUSED
    return out, src


def check_load_records(before, after, hdr, slot_pos, src, *, alt=False, status=None, allow_empty=False):
    """Pure CPU.  cw_load_records(src, hdr [R, 16], slot_pos [R, 8]) ran between the snapshots `before` and `after` (masked_check.take()); src: the N
    entries the kernel read, or None; status: the bytes it wrote, or None; alt: the engine's raster is AltObs.
    An env that LOADS (0 <= src[i] < R and record_rule accepts the record): hdr equals the record's but byte 3, which is the env's own; slot_pos the
    record's; state_grid / agent_rc / hold / achieved / desired / step_num what the record decodes to; achieved_mask / desired_mask the record's masks; in
    the pixel modes `observation` the oracle's frame of the decoded state.  EVERYTHING ELSE -- the start and goal states and their frames, ep_no, the
    streams, reward, done, the episode outputs of a loaded env, and every entry of every other env -- is byte for byte as before.  counters: [6] = before
    + the envs with an index at or above R or a refused record, every other word as before.  status == the expected bytes.
    ValueError when no env loads (nothing would be compared with a record) unless allow_empty.  -> the expected status bytes."""
    if set(before) != set(after):
        raise ValueError('the snapshots hold different entries: %s' % sorted(set(before) ^ set(after)))
    N, S = len(before['rng_pos']), before['state_grid'].shape[1]
    hdr = np.ascontiguousarray(hdr, dtype=np.uint8).reshape(-1, 16)
    pos = np.ascontiguousarray(slot_pos).reshape(-1, 8).view(np.uint16)
    if len(hdr) != len(pos):
        raise ValueError('%d headers, %d slot records' % (len(hdr), len(pos)))
    want_status, src = expected_status(N, len(hdr), S, hdr, pos, src)
    good = np.flatnonzero(want_status == LOADED)
    if len(good) == 0 and not allow_empty:
        raise ValueError('no env loads a record: nothing would be compared with one (allow_empty=True if that is the case under test)')
    want = {k: v.copy() for k, v in before.items()}
    if len(good):
        rec = src[good]
        d = decode(hdr[rec], pos[rec], S)
        want['hdr'][good] = hdr[rec]
        want['hdr'][good, 3] = before['hdr'][good, 3]
        want['slot_pos'][good] = pos[rec].view(want['slot_pos'].dtype)
        for k, f in (('state_grid', 'grid'), ('state_agent_rc', 'agent'), ('state_hold', 'hold'), ('state_achieved', 'achieved'),
                     ('state_desired', 'desired'), ('state_step_num', 'step_num')):
            want[k][good] = d[f].astype(want[k].dtype)
        want['achieved_mask'][good] = d['achieved'].astype(np.uint16).view(want['achieved_mask'].dtype)
        want['desired_mask'][good] = d['desired'].astype(np.uint16).view(want['desired_mask'].dtype)
        if 'observation' in before:
            want['observation'][good] = np.stack([oracle_frame(d['grid'][j], d['agent'][j], d['hold'][j], alt) for j in range(len(good))])
    want['counters'][SKIPPED] += int(((want_status == BAD_INDEX) | (want_status == REFUSED)).sum())
    for k in sorted(before):
        if k == 'counters':
            assert np.array_equal(after[k], want[k]), 'counters after a record load: %s, expected %s' % (after[k].tolist(), want[k].tolist())
        else:
            same('after a record load: ' + k, 0, after[k], want[k])
    if status is not None:
        same('status', 0, np.asarray(status).reshape(-1).astype(np.uint8), want_status)
    return want_status
