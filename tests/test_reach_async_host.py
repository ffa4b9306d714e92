"""CPU tier: the host side of cw_reach -- the HIP-free argument rules (cw_host.h: cwh_reach_args) row by row, the workspace's size and sections
(cwh_reach_bytes_of, cwh_reach_layout) at their limits, the arithmetic of rows, chunks and grids at the edges of a wave and a chunk against
tests/reach_check.py, the ctypes mirror of cw_reach_out against the C compiler's layout, and the ABI entries."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from hostlib import host_lib
from reach_check import CHUNK, padded, rows_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = 1 << 20                                     # an address: 16-byte aligned, far from 0


@pytest.fixture(scope='module')
def lib():
    return host_lib()


def test_reach_args_row_by_row(lib):
    L, h = lib
    m, d, n = 100, 7, 100
    hdr, pos, eo = A, A + 16 * m, A + 32 * m
    dist, plan, first, front, srch = A + 36 * m, A + 40 * m, A + 40 * m + d * m, A + 41 * m + d * m, A + 41 * m + d * m + 4 * d      # back to back, nothing shared
    ok = lambda *a: h.cwh_reach_args(*a)  # noqa: E731
    full = (dist, plan, first, front, srch)
    assert ok(n, eo, hdr, pos, m, d, *full) == L.CWH_REACH_OK
    assert ok(n, 0, hdr, pos, m, d, *full) == L.CWH_REACH_OK and ok(n, 0, 0, 0, n, d, *full) == L.CWH_REACH_OK           # env j % num_envs; the engine's own records
    for k in range(5):                                                                                                   # any one field alone
        assert ok(n, eo, hdr, pos, m, d, *[full[i] if i == k else 0 for i in range(5)]) == L.CWH_REACH_OK
    assert ok(n, eo, hdr, pos, 0, d, *full) == L.CWH_REACH_OK and ok(n, eo, hdr, pos, m, 1, *full) == L.CWH_REACH_OK
    assert ok(n, 0, hdr, pos, L.CWH_REACH_MAX_ROWS, L.CWH_REACH_MAX_DEPTH, 0, 0, 0, 1 << 50, 1 << 51) == L.CWH_REACH_OK
    assert ok(n, eo, hdr, pos, m, d, dist, plan + 1, 0, front, srch) == L.CWH_REACH_OK                                   # plan and first_action are bytes: any alignment
    assert ok(n, eo, hdr, pos, m, d, dist, 0, first + 3, front, srch) == L.CWH_REACH_OVERLAP and ok(n, eo, hdr, pos, m, d, dist, 0, first - 1, 0, srch) == L.CWH_REACH_OK
    # in the order they are tested
    assert ok(n, eo, hdr, pos, m, d, 0, 0, 0, 0, 0) == L.CWH_REACH_NO_FIELD and ok(n, eo, hdr, 0, -1, 0, 0, 0, 0, 0, 0) == L.CWH_REACH_NO_FIELD
    assert ok(n, eo, hdr, pos, -1, d, *full) == L.CWH_REACH_N_STATES and ok(n, eo, hdr, pos, L.CWH_REACH_MAX_ROWS + 1, d, *full) == L.CWH_REACH_N_STATES
    assert ok(n, eo, hdr, 0, -1, 0, *full) == L.CWH_REACH_N_STATES
    assert ok(n, eo, hdr, pos, m, 0, *full) == L.CWH_REACH_DEPTH and ok(n, eo, hdr, pos, m, L.CWH_REACH_MAX_DEPTH + 1, *full) == L.CWH_REACH_DEPTH
    assert ok(n, eo, hdr, pos, m, -5, *full) == L.CWH_REACH_DEPTH and ok(n, eo, hdr, 0, m, 0, *full) == L.CWH_REACH_DEPTH
    assert ok(n, eo, hdr, 0, m, d, *full) == L.CWH_REACH_PAIR and ok(n, eo, 0, pos, m, d, *full) == L.CWH_REACH_PAIR
    assert ok(n, eo, 0, 0, n, d, *full) == L.CWH_REACH_ENV_OF and ok(n, eo, 0, 0, n + 1, d, *full) == L.CWH_REACH_ENV_OF
    assert ok(n, 0, 0, 0, n + 1, d, *full) == L.CWH_REACH_OWN_STATES and ok(n, 0, 0, 0, 0, d, *full) == L.CWH_REACH_OWN_STATES
    for bad in [(n, eo, hdr + 8, pos, m, d) + full, (n, eo, hdr, pos + 4, m, d) + full, (n, eo + 2, hdr, pos, m, d) + full,
                (n, eo, hdr, pos, m, d, dist + 1, plan, first, front, srch), (n, eo, hdr, pos, m, d, dist, plan, first, front + 2, srch),
                (n, eo, hdr, pos, m, d, dist, plan, first, front, srch + 3), (n, eo, hdr + 1, hdr, m, d, hdr, hdr, hdr, hdr, hdr)]:
        assert ok(*bad) == L.CWH_REACH_ALIGN, bad
    far = 1 << 40
    for bad in [(hdr, 0, 0, 0, 0), (hdr + 16 * m - 4, 0, 0, 0, 0), (0, pos + 5, 0, 0, 0), (0, 0, eo + 4 * m - 1, 0, 0), (0, 0, 0, eo, 0), (0, 0, 0, 0, hdr + 16),
                (dist, dist + 4 * m - 1, 0, 0, 0), (dist, 0, dist + 1, 0, 0), (0, plan, plan + d * m - 1, 0, 0), (0, 0, 0, front, front + 4 * d - 4),
                (dist, plan, first, front, front), (far, far + 4 * m - 4, 0, 0, 0), (0, plan, 0, plan + d * m - 4, 0)]:
        assert ok(n, eo, hdr, pos, m, d, *bad) == L.CWH_REACH_OVERLAP, bad
    assert ok(n, eo, hdr, pos, m, d, hdr - 4 * m, plan, first, front, front + 4 * d) == L.CWH_REACH_OK                   # touching is not sharing
    assert ok(n, 0, hdr, pos, m, d, 4, 0, 0, 0, 0) == L.CWH_REACH_OK                                                     # without env_of nothing overlaps address 0
    assert ok(n, eo, hdr, pos, 0, d, hdr, hdr, hdr, front, srch) == L.CWH_REACH_OK                                       # no rows: no bytes to share


def test_reach_bytes_of_at_its_limits(lib):
    L, h = lib
    assert L.CWH_REACH_MAX_ROWS == (2 ** 28 - 1) // 6 - 63 and 6 * (L.CWH_REACH_MAX_ROWS + 63) < 2 ** 28 <= 6 * (L.CWH_REACH_MAX_ROWS + 64)
    for bad in [(0, 5), (-1, 5), (L.CWH_REACH_MAX_ROWS + 1, 5), (100, 0), (100, -1), (100, L.CWH_REACH_MAX_DEPTH + 1), (2 ** 62, 5)]:
        assert h.cwh_reach_bytes_of(*bad) == -1, bad
    top = h.cwh_reach_bytes_of(L.CWH_REACH_MAX_ROWS, L.CWH_REACH_MAX_DEPTH)
    assert 4 * L.CWH_REACH_MAX_ROWS * (L.CWH_REACH_MAX_DEPTH - 1) < top < 2 ** 43                     # far inside int64
    assert rows_of(L.CWH_REACH_MAX_ROWS) < 2 ** 28                                                     # the row field of the set's bids
    for rows, depth in [(1, 1), (1, 9), (60, 10), (4096, 24), (2 ** 22, 24), (L.CWH_REACH_MAX_ROWS, 2)]:
        at = (C.c_uint64 * L.CWH_REACH_SECTIONS)()
        total = h.cwh_reach_layout(rows, depth, at)
        assert total == h.cwh_reach_bytes_of(rows, depth) > 0
        n, chunks = rows_of(rows), (rows_of(rows) + CHUNK - 1) // CHUNK
        want = [4 * (64 + depth + 1 + chunks)] + [16 * rows, 16 * rows, 4 * rows, 4 * rows] * 2 + [16 * n, 16 * n, 4 * n, chunks * CHUNK, 4 * rows * (depth - 1),
                                                                                                   4 * rows, 4 * rows, 4 * rows, rows]
        assert len(want) == L.CWH_REACH_SECTIONS
        ends = list(at[1:]) + [total]
        for i in range(L.CWH_REACH_SECTIONS):
            assert at[i] % 256 == 0 and ends[i] - at[i] >= want[i] and ends[i] - at[i] < want[i] + 256, (rows, depth, i)
        assert total <= rows * (80 + 6 * 37 + 13 + 4 * (depth - 1)) + 64 * 37 * 6 + CHUNK + 4 * (65 + depth + chunks) + 256 * L.CWH_REACH_SECTIONS
    assert h.cwh_reach_bytes_of(100, 5) < h.cwh_reach_bytes_of(100, 6) and h.cwh_reach_bytes_of(100, 5) < h.cwh_reach_bytes_of(200, 5)


def test_rows_chunks_and_grids_at_the_edges(lib):
    L, h = lib
    assert L.CWH_REACH_CHUNK == CHUNK == 256 * 16
    for F in [0, 1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 10 ** 6 + 1]:
        assert h.cwh_reach_rows_of(F) == rows_of(F) == 6 * padded(F)
    for rows, chunks in [(0, 0), (1, 1), (CHUNK - 1, 1), (CHUNK, 1), (CHUNK + 1, 2), (7 * CHUNK, 7), (7 * CHUNK + 1, 8)]:
        assert h.cwh_reach_chunks_of(rows) == chunks
    # the chunks of a level over F states, F at the edges of a chunk: 6 * padded(F) rows
    assert [h.cwh_reach_chunks_of(h.cwh_reach_rows_of(F)) for F in (0, 1, CHUNK - 1, CHUNK, CHUNK + 1)] == [0, 1, 6, 6, 7]
    most = 256 * L.CWH_REACH_BLOCKS_PER_CU
    assert [h.cwh_reach_grid_of(i, 256) for i in (0, 1, 256, 257, 256 * most, 256 * most + 1, 2 ** 28)] == [1, 1, 1, 2, most, most, most]
    assert h.cwh_reach_grid_of(10 ** 9, 1) == L.CWH_REACH_BLOCKS_PER_CU and h.cwh_reach_grid_of(1000, 304) == 4


def test_reach_out_mirror_matches_the_header_and_the_abi_names_the_calls(lib, tmp_path):
    L, h = lib
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "craftingworld.h"', 'int main(void){', 'printf("size %zu\\n", sizeof(cw_reach_out));']
    for f, _ in L.cw_reach_out._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(cw_reach_out, %s));' % (f, f))
    lines.append('return 0;}')
    src, exe = tmp_path / 'reach.c', tmp_path / 'reach'
    src.write_text('\n'.join(lines))
    subprocess.check_call(['gcc', '-std=c99', '-pedantic', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got['size']) == C.sizeof(L.cw_reach_out)
    for f, _ in L.cw_reach_out._fields_:
        assert int(got[f]) == getattr(L.cw_reach_out, f).offset
    if not os.environ.get('CW_HOST_LIB'):
        for name in ('cw_reach_reserve', 'cw_reach_bytes', 'cw_reach'):
            assert name in L.ABI and hasattr(h, name), name
        from gym_craftingworld_amd.vec_env import REACH_FIELDS, REACH_MAX_ROWS
        assert REACH_FIELDS == tuple(f for f, _ in L.cw_reach_out._fields_) and REACH_MAX_ROWS == L.CWH_REACH_MAX_ROWS
        hdr = open(os.path.join(ROOT, 'include', 'craftingworld.h')).read()
        assert 'cw_reach_out, cw_reach_reserve, cw_reach_bytes, cw_reach;' in hdr.split('#define CW_MT_N')[0] and '#define CW_ABI_VERSION 5 ' in hdr


_ASAN_MAIN = r'''
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "cw_host.h"
int main()
{
    unsigned long long sum = 0;
    const int64_t rows[] = {INT64_MIN, -1, 0, 1, 63, 64, 65, 4095, 4096, 4097, 1 << 22, CWH_REACH_MAX_ROWS, CWH_REACH_MAX_ROWS + 1, INT64_MAX};
    const int32_t depths[] = {INT32_MIN, -1, 0, 1, 2, 24, CWH_REACH_MAX_DEPTH, CWH_REACH_MAX_DEPTH + 1, INT32_MAX};
    for (int64_t r : rows) for (int32_t d : depths) {
        std::vector<uint64_t> at(CWH_REACH_SECTIONS);                  // exactly sized: a write past the last section's offset is an ASAN report
        const int64_t total = cwh_reach_layout(r, d, at.data());
        if (total != cwh_reach_bytes_of(r, d)) return 2;
        if (total >= 0 && at[CWH_REACH_SECTIONS - 1] >= (uint64_t)total) return 3;
        sum += (unsigned long long)total;
    }
    for (int64_t f : rows) if (f >= 0 && f <= CWH_REACH_MAX_ROWS) sum += (unsigned long long)(cwh_reach_chunks_of(cwh_reach_rows_of(f)) + cwh_reach_grid_of(f, 256));
    const uint64_t at[] = {0, 3, 16, 1ull << 20, (1ull << 20) + 4, UINT64_MAX - 15, UINT64_MAX};
    const int32_t ns[] = {INT32_MIN, -1, 0, 1, 100, (int32_t)CWH_REACH_MAX_ROWS, INT32_MAX};
    for (uint64_t e : at) for (uint64_t h : at) for (uint64_t p : at) for (int32_t n : ns) for (int32_t d : depths) for (uint64_t o : at) for (uint64_t q : at)
        sum += (unsigned long long)cwh_reach_args(100, e, h, p, n, d, o, q, o, q, o);
    if (cwh_reach_args(100, 0, 1ull << 20, 1ull << 21, 100, CWH_REACH_MAX_DEPTH, UINT64_MAX - 15, 0, 0, 0, 0) != CWH_REACH_OK) return 4;     // a range that would wrap ends at the top
    printf("ok %llu\n", sum);
    return 0;
}
'''


def test_the_host_side_under_asan_and_ubsan(tmp_path):
    """cw_host.cpp and a stand-alone program that drives the cwh_reach_* functions, both built with -fsanitize=address,undefined: the size rule and the
    sections at and beyond both limits into an exactly sized array, and the argument rules over addresses at both ends of the address space"""
    csrc = os.path.join(ROOT, 'gym_craftingworld_amd', 'csrc')
    src, exe = tmp_path / 'reach_main.cpp', tmp_path / 'reach_main'
    src.write_text(_ASAN_MAIN)
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                           '-fno-omit-frame-pointer', '-I', csrc, str(src), os.path.join(csrc, 'cw_host.cpp'), '-o', str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0'), timeout=120)
    assert p.returncode == 0 and p.stdout.startswith('ok '), (p.returncode, p.stdout[-500:], p.stderr[-3000:])
    assert 'runtime error' not in p.stderr and 'AddressSanitizer' not in p.stderr, p.stderr[-3000:]
