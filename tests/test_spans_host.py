"""CPU tier: the two primitives under the host-side rules (cw_host.h) -- the span checker (cwh_spans_misaligned, cwh_spans_clash), which every entry point's
alignment and overlap rule goes through, against a model of sets of byte addresses, and the section layout (cwh_sections_layout) with the four layouts built on
it -- and the stand-alone program that repeats the brute force under ASAN and UBSAN (tests/host/spans_check.cpp, make host_check)."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

from hostlib import host_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOP = 2 ** 64 - 1


@pytest.fixture(scope='module')
def lib():
    return host_lib()


def _spans(L, rows):
    return (L.cwh_span * max(len(rows), 1))(*[L.cwh_span(*r) for r in rows])


def _clash(L, h, outs, ins, among):
    other = C.c_int(-7)
    o = h.cwh_spans_clash(_spans(L, outs), len(outs), _spans(L, ins), len(ins), among, C.byref(other))
    return o, other.value


# ---- the clash function against sets of byte addresses: addresses 0 (not given), 8 .. 15, 0 .. 4 bytes, so a span's set is a bit mask of the addresses 8 .. 18
PAIRS = [(a, b) for a in (0,) + tuple(range(8, 16)) for b in range(5)]
BYTE_SET = np.array([0 if a == 0 else ((1 << b) - 1) << a for a, b in PAIRS], np.int64)
PAIR_ROWS = np.array([(a, b, 1) for a, b in PAIRS], np.uint64)
# the product is full up to three spans (every (address, bytes) pair of an output against every pair of an input and of a later output, with every third
# span beside them); of the 45^4 combinations of two outputs and two inputs every THIN-th is kept, a stride prime to 45 so that it walks through every pair
# at every place
THIN = 41


def _combinations(n_spans):
    idx = np.indices((len(PAIRS),) * n_spans).reshape(n_spans, -1).T if n_spans else np.zeros((1, 0), np.int64)
    return np.ascontiguousarray(idx[::THIN] if n_spans == 4 else idx)


def _model(idx, n_outs, n_ins, among):
    """-> (output, other) per row of idx, the first pair in cwh_spans_clash's order whose byte sets meet; (-1, -7): none"""
    sets = BYTE_SET[idx]
    o_hit, other = np.full(len(idx), -1), np.full(len(idx), -7)
    order = [(o, n_outs + i, i) for o in range(n_outs) for i in range(n_ins)]
    order = sorted(order + [(o, q, n_ins + q) for o in range(n_outs) for q in range(o + 1, n_outs) if among],
                   key=lambda t: (t[0], t[2]))                          # per output: the inputs in order, then the later outputs in order
    for o, column, reported in reversed(order):
        meet = (sets[:, o] & sets[:, column]) != 0
        o_hit[meet], other[meet] = o, reported
    return o_hit, other


def test_clash_against_sets_of_byte_addresses(lib):
    L, h = lib
    fn = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int))(('cwh_spans_clash', h))     # (addresses into one table)
    other = C.c_int()
    cases = 0
    for n_outs, n_ins in itertools.product(range(3), range(3)):
        idx = _combinations(n_outs + n_ins)
        table = np.ascontiguousarray(PAIR_ROWS[idx])                    # [case][span][at, bytes, align]: the outputs, then the inputs
        assert table.dtype == np.uint64 and C.sizeof(L.cwh_span) == 24
        base, stride = table.ctypes.data, 24 * (n_outs + n_ins)
        for among in (0, 1):
            want_o, want_other = _model(idx, n_outs, n_ins, among)
            got_o, got_other = [], []
            for k in range(len(idx)):
                other.value = -7
                got_o.append(fn(base + k * stride, n_outs, base + k * stride + 24 * n_outs, n_ins, among, other))
                got_other.append(other.value)
            bad = np.flatnonzero((np.array(got_o) != want_o) | (np.array(got_other) != want_other))
            assert len(bad) == 0, (n_outs, n_ins, among, [PAIRS[p] for p in idx[bad[0]]], got_o[bad[0]], got_other[bad[0]], want_o[bad[0]], want_other[bad[0]])
            cases += len(idx)
    assert cases > 500000
    for o_pair, i_pair in itertools.product(range(len(PAIRS)), repeat=2):                       # (what the thinning must not lose, spelled out)
        want = 0 if BYTE_SET[o_pair] & BYTE_SET[i_pair] else -1
        assert _clash(L, h, [tuple(PAIR_ROWS[o_pair])], [tuple(PAIR_ROWS[i_pair])], 0)[0] == want
        assert _clash(L, h, [tuple(PAIR_ROWS[o_pair]), tuple(PAIR_ROWS[i_pair])], [], 1) == ((0, 1) if want == 0 else (-1, -7))


def test_clash_order_and_the_reported_pair(lib):
    L, h = lib
    a, b, c, d = (64, 16, 1), (72, 16, 1), (200, 8, 1), (204, 8, 1)
    assert _clash(L, h, [a, c], [d, b], 1) == (0, 1)                    # output 0 first, though output 1 meets input 0
    assert _clash(L, h, [c, a], [d, b], 1) == (0, 0)
    assert _clash(L, h, [a, b, c], [d], 1) == (0, 1 + 1)                # a later output is reported behind the inputs: n_ins + q
    assert _clash(L, h, [a, b, c], [d], 0) == (2, 0)                    # ... and not at all without the flag
    assert _clash(L, h, [a, b], [b], 1) == (0, 0)                       # the inputs before the later outputs
    assert _clash(L, h, [(0, 16, 1), a], [(0, 16, 1), a], 1) == (1, 1)  # not given: never, on either side
    assert _clash(L, h, [(64, 0, 1), a], [a], 1) == (1, 0)              # no bytes: never
    assert _clash(L, h, [a], [(80, 16, 1)], 1) == (-1, -7) and _clash(L, h, [], [a], 1) == (-1, -7)       # touching is not sharing; *other is left alone
    assert h.cwh_spans_clash(_spans(L, [a]), 1, _spans(L, [b]), 1, 0, None) == 0                # *other may be null


def test_saturation_is_cwh_ranges_overlaps(lib):
    L, h = lib
    spans = [(TOP - 15, 15, 1), (TOP - 15, 16, 1), (TOP - 15, 1000, 1), (TOP, 1, 1), (TOP, TOP, 1), (TOP - 1, 1, 1), (16, TOP, 1), (16, 16, 1), (1, TOP, 1),
             (TOP - 16, 1, 1), (TOP - 16, 2, 1)]
    seen = set()
    for x, y in itertools.product(spans, repeat=2):
        want = h.cwh_ranges_overlap(x[0], x[1], y[0], y[1])
        seen.add(want)
        assert _clash(L, h, [x], [y], 0) == ((0, 0) if want else (-1, -7)), (x, y)
        assert _clash(L, h, [x, y], [], 1) == ((0, 1) if want else (-1, -7)), (x, y)
    assert seen == {0, 1}
    assert h.cwh_ranges_overlap(TOP - 15, 15, TOP, 1) == 0 and h.cwh_ranges_overlap(TOP - 15, 1000, TOP - 1, 1) == 1      # ends at 2^64 - 1; wraps: saturates


def test_misaligned_names_the_first_offender(lib):
    L, h = lib
    rows = [(0, 8, 16), (32, 8, 16), (33, 8, 1), (33, 8, 0), (34, 8, 2), (36, 8, 8), (35, 8, 2)]
    mis = lambda r, n=None: h.cwh_spans_misaligned(_spans(L, r), len(r) if n is None else n)  # noqa: E731
    assert mis(rows) == 5 and mis(rows, 5) == -1 and mis(rows, 0) == -1
    assert mis(rows[:5] + [(0, 8, 8)] + rows[6:]) == 6                  # a span that is not given is skipped
    assert mis([(3, 8, 16)]) == 0 and mis([(0, 8, 16), (0, 0, 4)]) == -1
    for at in range(1, 70):
        assert mis([(at, 0, 1)]) == -1                                  # alignment 1 never offends
        for align in (2, 4, 16):
            assert mis([(at, 4, align)]) == (0 if at % align else -1), (at, align)
    assert mis([(TOP, 1, 1), (TOP - 15, 1, 16), (TOP - 14, 1, 16)]) == 2


def _layout(h, sizes, align):
    n = len(sizes)
    at = (C.c_uint64 * max(n, 1))()
    total = h.cwh_sections_layout((C.c_uint64 * max(n, 1))(*sizes), n, align, at)
    assert h.cwh_sections_layout((C.c_uint64 * max(n, 1))(*sizes), n, align, None) == total
    return list(at)[:n], total


def _assert_layout(at, total, sizes, align):
    rounded = [(b + align - 1) // align * align for b in sizes]
    assert at == [sum(rounded[:i]) for i in range(len(sizes))] and total == sum(rounded)
    assert all(x % align == 0 for x in at) and all(x <= y for x, y in zip(at, at[1:]))


def test_sections_layout(lib):
    _, h = lib
    r = np.random.RandomState(5)
    for align in (1, 2, 16, 256, 4096):
        for sizes in ([], [0], [1], [align], [align + 1, 0, 0, 3], list(r.randint(0, 5000, 16)), [2 ** 40 + 1, 7, 2 ** 33]):
            sizes = [int(s) for s in sizes]
            _assert_layout(*_layout(h, sizes, align), sizes, align)


def test_the_four_layouts_are_the_section_layout(lib):
    L, h = lib
    for rows, k, la in ((3, 0, 0), (1000, 3, 4)):
        sizes, at = (C.c_size_t * L.CWH_SNAP_SECTIONS)(), (C.c_size_t * L.CWH_SNAP_SECTIONS)()
        total = C.c_uint64()
        assert h.cwh_snapshot_section_bytes(rows, k, la, sizes, at, C.byref(total), None) == L.CWH_SNAP_SECTIONS
        assert (list(at), total.value) == _layout(h, list(sizes), L.CWH_SNAP_ALIGN)
        _assert_layout(list(at), total.value, list(sizes), L.CWH_SNAP_ALIGN)
    for steps, n in ((1, 1), (1000, 37)):
        t = steps * n
        at = (C.c_uint64 * L.CWH_REPLAY_SECTIONS)()
        total = h.cwh_replay_layout(steps, n, at)
        assert (list(at), total) == _layout(h, [L.CWH_REPLAY_CTL_BYTES, 4 * n] + [16 * t] * 6 + [4 * t, 4 * t, t, t], L.CWH_SNAP_ALIGN)
    for rows, depth in ((1, 1), (5000, 9)):
        at = (C.c_uint64 * L.CWH_REACH_SECTIONS)()
        total = h.cwh_reach_layout(rows, depth, at)
        lvl = h.cwh_reach_rows_of(rows)
        chunks = h.cwh_reach_chunks_of(lvl)
        sizes = [4 * (64 + depth + 1 + chunks)] + [16 * rows, 16 * rows, 4 * rows, 4 * rows] * 2 + [16 * lvl, 16 * lvl, 4 * lvl, chunks * L.CWH_REACH_CHUNK,
                                                                                                     4 * rows * (depth - 1), 4 * rows, 4 * rows, 4 * rows, rows]
        assert (list(at), total) == _layout(h, sizes, L.CWH_SNAP_ALIGN)


def test_seen_layout(lib):
    L, h = lib
    for n in (2, 4, 2048):
        at = (C.c_uint64 * L.CWH_SEEN_SECTIONS)()
        assert h.cwh_seen_layout(n, at) == 256 + 48 * n and h.cwh_seen_layout(n, None) == 256 + 48 * n
        assert list(at) == [0, 256, 256 + 8 * n, 256 + 16 * n, 256 + 32 * n]
        assert (list(at), 256 + 48 * n) == _layout(h, [L.CWH_SEEN_CTL_BYTES, 8 * n, 8 * n, 16 * n, 16 * n], 16)
    # accepted: exactly the slot counts cwh_seen_slots_of gives a set
    legal = {h.cwh_seen_slots_of(c) for c in list(range(1, 600)) + [2 ** k + d for k in range(9, 29) for d in (-1, 0, 1)] if c <= L.CWH_SEEN_MAX_CAPACITY}
    assert legal == {2 ** k for k in range(1, 30)} and h.cwh_seen_slots_of(0) == 0
    for n in sorted(legal) + [0, 1, 3, 6, 1000, 2 ** 29 - 1, 2 ** 29 + 1, 2 ** 30, 2 ** 62, -1, -2, -2 ** 63]:
        assert h.cwh_seen_layout(n, None) == (256 + 48 * n if n in legal else -1), n


def test_the_stand_alone_check_under_asan_and_ubsan(tmp_path):
    """tests/host/spans_check.cpp with cw_host.cpp, both built with -fsanitize=address,undefined (make host_check): the same brute force in full against a
    byte-set model in C++ on exactly-sized heap arrays, saturation, misalignment, and the seen and replay layouts at their largest legal arguments"""
    exe = tmp_path / 'spans_check'
    subprocess.check_call(['make', '-C', os.path.join(ROOT, 'gym_craftingworld_amd', 'csrc'), 'host_check', 'HOST_CHECK=%s' % exe], stdout=subprocess.DEVNULL)
    p = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0'), timeout=120)
    assert p.returncode == 0 and p.stdout.startswith('ok '), (p.returncode, p.stdout[-500:], p.stderr[-3000:])
    assert int(p.stdout.split()[1]) == 2 * sum(45 ** (o + i) for o in range(3) for i in range(3))
    assert 'runtime error' not in p.stderr and 'AddressSanitizer' not in p.stderr, p.stderr[-3000:]
