"""What "a snapshot call did exactly what it should" means for cw_snapshot_save / cw_snapshot_load, in one place.  Both checkers work on
masked_check.take() snapshots -- numpy arrays, no GPU: check_save compares the engine before and after a save (nothing may have changed), check_load
compares the engine before and after a load with the snapshot taken when the rows were saved: EVERY env with a good row against its saved source,
every other env byte for byte against the before-snapshot, and the skipped envs against counters[6].  A plain module, not a fixture;
tests/test_snapshot_logic.py tests the comparison itself, on the CPU."""
import numpy as np

from oracle_replay import FRAMES, same

UNTOUCHED_OUTPUTS = ('reward', 'done', 'episode_length', 'episode_return')     # a restore is not a step and not a finished episode
SKIPPED = 6                                                                    # counters[6]: envs skipped for a bad row number


def sources(save_rows, capacity):
    """-> {bank row: the env saved into it} of a save with the row numbers `save_rows` [N] into a bank of `capacity` rows (negative: the env took no part,
    at or above the capacity: skipped).  ValueError when two envs name one row: what the row then holds is unspecified, nothing could be checked."""
    out = {}
    for i, r in enumerate(np.asarray(save_rows).reshape(-1).tolist()):
        if 0 <= r < capacity:
            if r in out:
                raise ValueError('envs %d and %d were saved into row %d' % (out[r], i, r))
            out[r] = i
    return out


def check_save(before, after):
    """a save writes nothing of the engine but the bank: the snapshots are equal everywhere, the counters included"""
    if set(before) != set(after):
        raise ValueError('the snapshots hold different entries: %s' % sorted(set(before) ^ set(after)))
    for k in sorted(before):
        if k == 'counters':
            assert np.array_equal(after[k], before[k]), 'counters changed by a save: %s -> %s' % (before[k].tolist(), after[k].tolist())
        else:
            same('after a save: ' + k, 0, after[k], before[k])


def check_load(saved, before, after, save_rows, load_rows, with_stream, capacity, allow_empty=False):
    """Pure CPU.  `saved`: take() when cw_snapshot_save(save_rows) ran; `before` / `after`: take() around cw_snapshot_load(load_rows, with_stream); the bank
    has `capacity` rows and held nothing else (reserved just before that save).
    Env i with a GOOD row (0 <= load_rows[i] < capacity, saved by env s): every state_* field, hdr, slot_pos and the three frames equal the saved
    source's; achieved_mask / desired_mask the source's saved masks; rng_key / rng_pos and hdr byte 3 (the menu id) the source's when with_stream, else the
    env's own before-values; reward, done, episode_length, episode_return as before.  Every other env -- no part (negative), row outside the bank, row
    never saved -- byte for byte as before.  counters: [6] = before + the envs with a bad row, every other word as before.
    Raises ValueError when no env has a good row (nothing would be compared with a source) unless allow_empty.  -> (envs with a good row, bad rows)."""
    if not set(saved) == set(before) == set(after):
        raise ValueError('the snapshots hold different entries')
    N = len(before['rng_pos'])
    load_rows = np.asarray(load_rows).reshape(-1)
    if len(load_rows) != N or len(np.asarray(save_rows).reshape(-1)) != N:
        raise ValueError('one row number per env (%d) on either side' % N)
    src_of = sources(save_rows, capacity)
    good = np.array([i for i in range(N) if int(load_rows[i]) in src_of and 0 <= load_rows[i] < capacity], dtype=np.int64)
    src = np.array([src_of[int(load_rows[i])] for i in good], dtype=np.int64)
    n_bad = int(((load_rows >= 0)).sum()) - len(good)
    if len(good) == 0 and not allow_empty:
        raise ValueError('no env loads a saved row: nothing would be compared with a source (allow_empty=True if that is the case under test)')
    want = {k: v.copy() for k, v in before.items()}
    if len(good):
        for k in before:
            if k.startswith('state_') or k in ('hdr', 'slot_pos') or k in FRAMES:
                want[k][good] = saved[k][src]
        want['achieved_mask'][good] = saved['state_achieved'][src].astype(want['achieved_mask'].dtype)
        want['desired_mask'][good] = saved['state_desired'][src].astype(want['desired_mask'].dtype)
        if with_stream:
            want['rng_key'][good], want['rng_pos'][good] = saved['rng_key'][src], saved['rng_pos'][src]
        else:
            want['hdr'][good, 3] = before['hdr'][good, 3]
    want['counters'][SKIPPED] = before['counters'][SKIPPED] + n_bad
    for k in UNTOUCHED_OUTPUTS:
        assert np.array_equal(want[k], before[k])
    for k in sorted(before):
        if k == 'counters':
            assert np.array_equal(after[k], want[k]), 'counters after a load with %d bad rows: %s, expected %s' % (n_bad, after[k].tolist(), want[k].tolist())
        else:
            same('after a load: ' + k, 0, after[k], want[k])
    return good, n_bad
