"""CPU tier of the sweep's chunk rule (csrc/cw_host.h: cwh_piece_chunks, the code cw_launch_sweep runs, called here through its exported twin
cwh_piece_chunks_of).  render_pieces and cw_render_gather_kernel index a chunk of a frame array with 32-bit offsets and round its bytes up to whole 4-KiB
pieces, so the rule alone stands between a large array and a wrapped offset.  Every grid size, both rasters, and batch sizes on both sides of 2^31 and 2^32
bytes; the launches of the shapes whose chunking was right before the rule was mended are pinned as literals, and the rule as it stood before is
restated here and must fail the same checks where it was wrong.  No torch, no GPU; what the kernels paint past 2^32 bytes is tests/test_big_arrays.py's."""
import ctypes as C

import pytest

from hostlib import host_lib

PIECE = 4096
LIMIT = 2 ** 32 - PIECE          # a chunk's bytes: total + PIECE - 1 (the piece count) and a0 + PIECE (a piece's end) are 32-bit sums in the kernels
INT32_MAX = 2 ** 31 - 1
SIZES = range(4, 256)
N_CU = (256, 304)
ROUNDS = (0, 1, 150, 896, INT32_MAX)


def frame_bytes(S, raster):
    return 27 * S * (S + 1) if raster == 'alt' else 48 * S * S


def batch_sizes(FB):
    """the batch sizes of the sweep for frames of FB bytes: small ones, around 4 096, around 2^31 and 2^32 bytes, past twice that, and the largest of the suite"""
    at32, at31 = 2 ** 32 // FB, 2 ** 31 // FB
    ns = {1, 4095, 4096, 4097, 131072, 2 * at32 + 1}
    for at in (at32, at31):
        ns |= {at - 1, at, at + 1, at + 4097}
    return sorted(n for n in ns if n >= 1)


@pytest.fixture(scope='module')
def rule():
    lib = host_lib()[1]

    def call(N, FB, n_cu, rounds):
        per = C.c_int(-1)
        chunks = lib.cwh_piece_chunks_of(N, FB, n_cu, rounds, C.byref(per))
        return chunks, per.value
    return call


def rule_before(N, FB, n_cu, rounds):
    """the rule as cw_kernels.hip held it before it moved to cw_host.h: chunks of whole multiples of 4 096 envs, never fewer"""
    cap = (rounds if rounds > 0 else 1 << 20) * n_cu * 4 * 3072
    n = max(1, -(-N * FB // cap))
    per = -(-N // n)
    if n > 1 or N * FB >= 2 ** 32:
        per = -(-per // 4096) * 4096
        while per * FB >= 2 ** 32 and per > 4096:
            per = -(-(per // 2) // 4096) * 4096
    return -(-N // per), per


def check(N, FB, chunks, per):
    """what the sweep's kernels need of (chunks, per) for N frames of FB bytes; chunk c covers envs [c * per, min(N, (c + 1) * per))"""
    what = (N, FB, chunks, per)
    assert per >= 1 and chunks == -(-N // per), what
    last = N - (chunks - 1) * per                       # (chunks 0 .. chunks - 2 hold per envs each: with 1 <= last <= per every env is covered exactly once)
    assert 1 <= last <= per and (chunks - 1) * per + last == N, what
    assert min(per, N) * FB < 2 ** 32, what             # the largest chunk
    assert min(per, N) * FB <= LIMIT, what              # ... and rounded up to whole pieces
    if chunks > 1:
        assert per * FB % PIECE == 0, what              # c * per * FB is then a multiple of 4 096 for every c


def test_every_size_raster_and_batch_on_both_sides_of_two_to_the_32(rule):
    """S = 4 .. 255, both rasters, 256 and 304 CUs, CW_TUNE_RENDER_CHUNK_ROUNDS from 0 to INT32_MAX, batch sizes around 2^31 and 2^32 bytes: the chunks cover
    every env exactly once, each holds at most 2^32 - 4096 bytes and starts on a 4-KiB boundary of the array; and wherever the rule as it stood before met
    all of that, the launches are the ones it gave."""
    cases = kept = 0
    for raster in ('ray', 'alt'):
        for S in SIZES:
            FB = frame_bytes(S, raster)
            for N in batch_sizes(FB):
                for n_cu in N_CU:
                    for rounds in ROUNDS:
                        chunks, per = rule(N, FB, n_cu, rounds)
                        check(N, FB, chunks, per)
                        cases += 1
                        before = rule_before(N, FB, n_cu, rounds)
                        try:
                            check(N, FB, *before)
                        except AssertionError:
                            continue
                        assert (chunks, per) == before, (N, FB, n_cu, rounds)
                        kept += 1
    assert cases == 10 * sum(len(batch_sizes(frame_bytes(S, r))) for S in SIZES for r in ('ray', 'alt')) >= 10 * (2 * 252 * 14 - 4)
    assert cases // 2 < kept < cases       # (14 batch sizes of nearly every frame; most shapes were right and stay as they were)


# (N, S, raster, rounds) -> (chunks, per) on 256 CUs, computed with the rule as it stood before: the shapes the suite's largest engines and the benchmark rely on
PINNED = {
    (65536, 21, 'ray', 150): (3, 24576),          # 24 576 + 24 576 + 16 384
    (65536, 32, 'ray', 350): (3, 24576),
    (65536, 21, 'ray', 896): (1, 65536),
    (65536, 32, 'ray', 896): (2, 32768),
    (131072, 21, 'ray', 896): (1, 131072),
    (65536, 21, 'alt', 896): (1, 65536),
    (65536, 8, 'ray', 896): (1, 65536),
    (65536, 5, 'ray', 896): (1, 65536),
    (90001, 32, 'ray', 896): (2, 45056),          # tests/test_big_arrays.py: two chunks for the rounds' sake, the second one ragged
    (90001, 32, 'ray', 0): (2, 45056),            # ... and by the halving loop: no limit on the rounds, 90 112 envs pass 2^32 bytes
    (1376, 255, 'ray', 896): (1, 4096),           # 4 294 771 200 bytes, the largest 255 x 255 batch that fits: one chunk (per >= N)
}


def test_launches_of_the_shapes_that_were_right_are_unchanged(rule):
    for (N, S, raster, rounds), want in PINNED.items():
        FB = frame_bytes(S, raster)
        assert rule(N, FB, 256, rounds) == want, (N, S, raster, rounds)
        assert rule_before(N, FB, 256, rounds) == want, (N, S, raster, rounds)      # (the literals are the earlier rule's)
        check(N, FB, *want)
    chunks, per = rule(65536, frame_bytes(21, 'ray'), 256, 150)
    assert [min(per, 65536 - c * per) for c in range(chunks)] == [24576, 24576, 16384]


# frames so large that 4 096 of them pass 2^32 bytes (Ray from 148 x 148, AltObs from 197 x 197): (N, S, raster) -> bytes of the array
WRONG_BEFORE = {(1377, 255, 'ray'): 4297892400, (4086, 148, 'ray'): 4295987712, (2437, 255, 'alt'): 4295358720}


@pytest.mark.parametrize('N,S,raster', sorted(WRONG_BEFORE))
def test_frames_of_which_4096_pass_two_to_the_32(rule, N, S, raster):
    """One chunk of all envs is what the rule gave before (the sweep's 32-bit `total` then wraps: 1 377 frames of 255 x 255 were swept as 2 925 104 bytes, less
    than one frame); the same checks that the rule passes now fail on it."""
    FB = frame_bytes(S, raster)
    assert N * FB == WRONG_BEFORE[N, S, raster] >= 2 ** 32 > (N - 1) * FB
    for n_cu in N_CU:
        for rounds in (0, 896):
            assert rule_before(N, FB, n_cu, rounds) == (1, 4096)
            with pytest.raises(AssertionError):
                check(N, FB, 1, 4096)
            chunks, per = rule(N, FB, n_cu, rounds)
            check(N, FB, chunks, per)
            assert chunks == 2 and per % (PIECE // _gcd(FB, PIECE)) == 0 and per < N
    if N == 1377:
        assert N * FB - 2 ** 32 == 2925104 < FB


def test_chunks_of_large_frames_follow_the_rounds_as_well(rule):
    """131 072 envs of 255 x 255 (409 GB): without a limit on the rounds as few chunks as 2^32 - 4096 bytes allow, 103 of 1 280 envs (five granules of 256); at
    the default 896 rounds (2.8 GB a launch) the 146 launches the rounds ask for, rounded up to whole granules: 128 of 1 024 envs"""
    FB = frame_bytes(255, 'ray')
    assert rule(131072, FB, 256, 0) == (103, 1280) and 1280 * FB <= LIMIT < 1536 * FB
    assert rule(131072, FB, 256, 896) == (128, 1024) and -(-131072 * FB // (896 * 1024 * 3072)) == 146
    assert rule(131072, FB, 256, 1) == (512, 256)           # never less than a granule


def _gcd(a, b):
    while b:
        a, b = b, a % b
    return a


def test_the_granule_of_the_largest_frames_fits_a_chunk():
    """4096 / gcd(frame_bytes, 4096) envs -- the fewest whose frames end on a 4-KiB boundary -- stay under the limit at every size: at most 256 envs of the Ray
    raster (frames are multiples of 16 bytes), at most 2 048 of AltObs (multiples of 2)"""
    for raster, most in (('ray', 256), ('alt', 2048)):
        granules = [PIECE // _gcd(frame_bytes(S, raster), PIECE) for S in SIZES]
        assert max(granules) == most
        assert all(g * frame_bytes(S, raster) <= LIMIT for g, S in zip(granules, SIZES))
    assert min(S for S in SIZES if 4096 * frame_bytes(S, 'ray') >= 2 ** 32) == 148
    assert min(S for S in SIZES if 4096 * frame_bytes(S, 'alt') >= 2 ** 32) == 197


def test_a_batch_within_4095_bytes_of_two_to_the_32_is_split(rule):
    """An array of more than 2^32 - 4096 and fewer than 2^32 bytes went as one chunk before: its piece count (total + 4095) / 4096 wraps in 32 bits just
    like a larger total.  Such batches exist (Ray 21 x 21: 202 899 frames end 1 264 bytes short of 2^32) and are split now."""
    found = []
    for raster in ('ray', 'alt'):
        for S in SIZES:
            FB = frame_bytes(S, raster)
            N = 2 ** 32 // FB
            if LIMIT < N * FB < 2 ** 32:
                found.append((S, raster))
                assert rule_before(N, FB, 256, 0) == (1, N)
                chunks, per = rule(N, FB, 256, 0)
                assert chunks == 2 and per % 4096 == 0
                check(N, FB, chunks, per)
    assert (21, 'ray') in found and 2 ** 32 - 202899 * frame_bytes(21, 'ray') == 1264
