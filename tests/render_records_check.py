"""What "a render_records call did exactly what it should" means for cw_render_records, in one place.  records_of() packs hand-built dense states into the
records the call reads, oracle_frames() paints them with the oracle's rasterisers, records_launch() restates the launch rule, and check_frames() compares
the WHOLE buffer an output array was a view of: every frame of a selected state byte for byte against the oracle's, every frame of a masked-out state and
every byte before and after the array against the sentinel the test pre-filled.  Pure CPU: numpy arrays in, no GPU.  A plain module, not a fixture;
tests/test_render_records_logic.py tests the comparison itself."""
import numpy as np

from records_check import encode
from state_tables import oracle_frame

CW_WAVE, WAVES_PER_BLOCK = 64, 4


def frame_shape(S, alt):
    return (3 * S + 3, 3 * S, 3) if alt else (4 * S, 4 * S, 3)


def frame_bytes(S, alt):
    return 27 * S * (S + 1) if alt else 48 * S * S


def records_launch(n_states, n_cu):
    """the shape cwk_launch_render_records gives cw_render_records_kernel (cw_render_grid: workgroups of four waves, at most one per CU) -> the waves of
    the launch; wave w paints states w, w + waves, ..."""
    return WAVES_PER_BLOCK * max(1, min((n_states + WAVES_PER_BLOCK - 1) // WAVES_PER_BLOCK, n_cu))


def dense_of(states):
    """painted_states()-style tuples (name, grid, init_grid, agent, hold) -> the dense fields records_check.encode takes (the masks and counters of a record
    do not matter to a painter: fixed values)"""
    n = len(states)
    z = np.zeros(n, np.int64)
    return dict(grid=np.stack([s[1] for s in states]), agent=np.array([s[3] for s in states], np.int64), hold=np.array([s[4] for s in states], np.int64),
                achieved=z, desired=z + 1, step_num=z + 2, flags=z)


def records_of(states):
    """-> (hdr uint8 [n, 16], slot_pos int16 [n, 8]) of painted_states()-style tuples"""
    hdr, pos = encode(dense_of(states))
    return hdr, pos.view(np.int16)


def oracle_frames(grid, agent, hold, alt):
    """the oracle's frame of each of n dense states -> uint8 [n, *frame_shape]"""
    return np.stack([oracle_frame(grid[j], agent[j], int(hold[j]), alt) for j in range(len(hold))])


def check_frames(buf, lo, want, mask, sentinel, allow_empty=False):
    """Pure CPU.  buf: uint8 [B], the whole buffer as it stands after the call, every byte of which was `sentinel` before it; the call's output array was
    the view buf[lo : lo + M * frame_bytes].  want: uint8 [M, ...], the oracle's frame of every state (masked-out ones included: they are not looked at);
    mask: None (every state) or the M bytes the kernel read (any non-zero byte selects).
    Every selected frame equals the oracle's byte for byte; every masked-out frame, the bytes before lo and the bytes after the array hold the sentinel.
    ValueError when no frame would be compared with the oracle (allow_empty=True if an empty selection is the case under test), for an array that does
    not fit the buffer, and for a sentinel an oracle frame could be made of.  -> the selected rows."""
    buf = np.asarray(buf)
    want = np.asarray(want)
    if buf.dtype != np.uint8 or buf.ndim != 1 or want.dtype != np.uint8 or want.ndim < 2:
        raise ValueError('buf must be uint8 [B] and want uint8 [M, ...]')
    M, fb = want.shape[0], int(np.prod(want.shape[1:]))
    if lo < 0 or lo + M * fb > len(buf):
        raise ValueError('an array of %d x %d bytes at %d does not fit a buffer of %d' % (M, fb, lo, len(buf)))
    sel = np.ones(M, bool) if mask is None else np.asarray(mask).reshape(-1).astype(np.uint8) != 0
    if len(sel) != M:
        raise ValueError('%d mask bytes for %d states' % (len(sel), M))
    rows = np.flatnonzero(sel)
    if len(rows) == 0 and not allow_empty:
        raise ValueError('nothing selected: nothing would be compared with the oracle')
    want = want.reshape(M, fb)
    if len(rows) and (want[rows] == sentinel).all(axis=1).any():
        raise ValueError('an expected frame consists of the sentinel alone: an unwritten frame would pass')
    got = buf[lo:lo + M * fb].reshape(M, fb)
    bad = rows[(got[rows] != want[rows]).any(axis=1)]
    if len(bad):
        j = int(bad[0])
        at = np.flatnonzero(got[j] != want[j])
        raise AssertionError('frames differ from the oracle at %d states, first %s; state %d: %d bytes, first at %d: %d, the oracle has %d'
                             % (len(bad), bad[:8].tolist(), j, len(at), at[0], got[j, at[0]], want[j, at[0]]))
    rest = np.flatnonzero(~sel)
    written = rest[(got[rest] != sentinel).any(axis=1)]
    assert len(written) == 0, 'frames of %d masked-out states were written, first %s' % (len(written), written[:8].tolist())
    before, after = np.flatnonzero(buf[:lo] != sentinel), np.flatnonzero(buf[lo + M * fb:] != sentinel)
    assert len(before) == 0, '%d bytes before the array were written, the last %d bytes before it' % (len(before), lo - before[-1])
    assert len(after) == 0, '%d bytes after the array were written, the first %d bytes past its end' % (len(after), after[0])
    return rows
