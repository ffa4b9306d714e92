"""CPU tier: the checker of the render_records tests (tests/render_records_check.py) itself.  The buffer a correct cw_render_records would leave is
synthesised on the CPU from the oracle's frames; the checker must accept it and must flag every kind of damage a wrong kernel could do."""
import numpy as np
import pytest

from render_records_check import check_frames, dense_of, frame_bytes, frame_shape, oracle_frames, records_launch, records_of
from state_tables import painted_states

SENT = 0xA5
S, LO, PAD = 5, 23, 40


def _correct(alt, mask):
    """-> (buf, want): what a correct call leaves in a sentinel-filled buffer whose bytes LO .. are the output array"""
    d = dense_of(painted_states(S))
    want = oracle_frames(d['grid'], d['agent'], d['hold'], alt)
    M, fb = len(want), frame_bytes(S, alt)
    assert want.shape[1:] == frame_shape(S, alt) and want[0].nbytes == fb
    buf = np.full(LO + M * fb + PAD, SENT, np.uint8)
    sel = np.ones(M, bool) if mask is None else np.asarray(mask) != 0
    out = buf[LO:LO + M * fb].reshape(M, fb)
    out[sel] = want.reshape(M, fb)[sel]
    return buf, want


def _alternating(M):
    return (np.arange(M) % 2 * 7).astype(np.uint8)              # (any non-zero byte selects)


@pytest.mark.parametrize('alt', [False, True])
def test_a_correct_buffer_passes(alt):
    buf, want = _correct(alt, None)
    assert len(check_frames(buf, LO, want, None, SENT)) == len(want)
    m = _alternating(len(want))
    buf, want = _correct(alt, m)
    assert check_frames(buf, LO, want, m, SENT).tolist() == list(range(1, len(want), 2))
    none = np.zeros(len(want), np.uint8)
    buf, want = _correct(alt, none)
    assert len(check_frames(buf, LO, want, none, SENT, allow_empty=True)) == 0


@pytest.mark.parametrize('alt', [False, True])
def test_one_wrong_byte_of_a_frame_is_flagged(alt):
    fb = frame_bytes(S, alt)
    for j, at in ((0, 0), (3, fb - 1), (21, fb // 2)):
        buf, want = _correct(alt, None)
        buf[LO + j * fb + at] ^= 1
        with pytest.raises(AssertionError, match='differ from the oracle at 1 states, first \\[%d\\]' % j):
            check_frames(buf, LO, want, None, SENT)
    buf, want = _correct(alt, None)                               # a frame left unwritten
    buf[LO + 2 * fb:LO + 3 * fb] = SENT
    with pytest.raises(AssertionError, match='first \\[2\\]'):
        check_frames(buf, LO, want, None, SENT)


@pytest.mark.parametrize('alt', [False, True])
def test_a_written_masked_out_row_is_flagged(alt):
    fb = frame_bytes(S, alt)
    m = _alternating(22)
    buf, want = _correct(alt, m)
    buf[LO + 4 * fb + 17] = 0                                     # one zero of the fill in the frame of state 4, which is masked out
    with pytest.raises(AssertionError, match='masked-out states were written, first \\[4\\]'):
        check_frames(buf, LO, want, m, SENT)
    buf, want = _correct(alt, None)                               # every frame written although the mask selects every other one
    with pytest.raises(AssertionError, match='masked-out'):
        check_frames(buf, LO, want, m, SENT)


@pytest.mark.parametrize('alt', [False, True])
def test_a_touched_guard_byte_is_flagged(alt):
    M, fb = 22, frame_bytes(S, alt)
    for at, word in ((LO - 1, 'before'), (0, 'before'), (LO + M * fb, 'after'), (LO + M * fb + PAD - 1, 'after')):
        buf, want = _correct(alt, None)
        buf[at] = 0
        with pytest.raises(AssertionError, match='bytes %s the array were written' % word):
            check_frames(buf, LO, want, None, SENT)


def test_it_refuses_to_compare_nothing():
    buf, want = _correct(True, None)
    none = np.zeros(len(want), np.uint8)
    with pytest.raises(ValueError, match='nothing selected'):
        check_frames(buf, LO, want, none, SENT)
    with pytest.raises(ValueError, match='mask bytes'):
        check_frames(buf, LO, want, none[:-1], SENT)
    with pytest.raises(ValueError, match='does not fit'):
        check_frames(buf[:-PAD - 1], LO, want, None, SENT)
    with pytest.raises(ValueError, match='sentinel alone'):
        check_frames(buf, LO, np.full_like(want, SENT), None, SENT)
    with pytest.raises(ValueError, match='uint8'):
        check_frames(buf.astype(np.int16), LO, want, None, SENT)


def test_records_of_packs_what_the_painter_reads():
    ps = painted_states(S)
    hdr, pos = records_of(ps)
    assert hdr.shape == (len(ps), 16) and hdr.dtype == np.uint8 and pos.shape == (len(ps), 8) and pos.dtype == np.int16
    for j, (_, grid, _, agent, hold) in enumerate(ps):
        assert (hdr[j, 0], hdr[j, 1], hdr[j, 2]) == (agent[0], agent[1], hold)
        p = pos[j].view(np.uint16)
        codes = [(hdr[j, 12 + k // 2] >> (4 * (k % 2))) & 15 for k in range(8)]
        on = [(int(p[k]), int(codes[k])) for k in range(8) if p[k] < S * S]
        assert sorted(on) == sorted((int(c), int(grid.reshape(-1)[c])) for c in np.flatnonzero(grid))
        assert sum(p[k] == 0xFFFE for k in range(8)) == (1 if hold else 0)


def test_the_launch_rule():
    assert [records_launch(m, 256) for m in (1, 4, 5, 63, 64, 65, 1024, 1025, 10 ** 6)] == [4, 4, 8, 64, 64, 68, 1024, 1024, 1024]
    assert records_launch(4 * 304 + 5, 304) == 4 * 304
