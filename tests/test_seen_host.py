"""CPU tier: the host side of the visited set -- the HIP-free argument rules of cw_seen_insert (cw_host.h: cwh_seen_args) row by row, the slot count of a
reserve (cwh_seen_slots_of), the key the kernels pack (cwh_seen_key_of) against tests/seen_check.key_of, the ctypes mirror of cw_seen_out against the C
compiler's layout, and the ABI entries."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from hostlib import host_lib
from seen_check import KEY_WORDS, key_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = 1 << 20                                     # an address: 16-byte aligned, far from 0


@pytest.fixture(scope='module')
def lib():
    return host_lib()


def test_seen_args_row_by_row(lib):
    L, h = lib
    m = 100
    hdr, pos, grp, fresh, first = A, A + 16 * m, A + 32 * m, A + 36 * m, A + 40 * m            # back to back, nothing shared
    ok = lambda *a: h.cwh_seen_args(*a)  # noqa: E731
    assert ok(grp, hdr, pos, m, fresh, first) == L.CWH_SEEN_OK
    assert ok(0, hdr, pos, m, fresh, first) == L.CWH_SEEN_OK                                    # no group: j % num_envs
    assert ok(grp, hdr, pos, m, fresh, 0) == L.CWH_SEEN_OK and ok(grp, hdr, pos, m, 0, first) == L.CWH_SEEN_OK      # either field alone
    assert ok(grp, hdr, pos, 0, fresh, first) == L.CWH_SEEN_OK and ok(grp, hdr, pos, L.CWH_MAX_STATES, 1 << 40, 1 << 41) == L.CWH_SEEN_OK
    assert ok(grp, hdr, pos, m, fresh + 1, first) == L.CWH_SEEN_OK                              # fresh is bytes: any alignment
    # in the order they are tested
    assert ok(grp, 0, pos, m, fresh, first) == L.CWH_SEEN_NO_RECORDS and ok(grp, hdr, 0, m, fresh, first) == L.CWH_SEEN_NO_RECORDS
    assert ok(grp, 0, pos, m, 0, 0) == L.CWH_SEEN_NO_RECORDS
    assert ok(grp, hdr, pos, m, 0, 0) == L.CWH_SEEN_NO_FIELD
    assert ok(grp, hdr, pos, -1, 0, 0) == L.CWH_SEEN_NO_FIELD
    assert ok(grp, hdr, pos, -1, fresh, first) == L.CWH_SEEN_N_STATES and ok(grp, hdr, pos, L.CWH_MAX_STATES + 1, fresh, first) == L.CWH_SEEN_N_STATES
    assert ok(grp, hdr + 8, pos, -1, fresh, first) == L.CWH_SEEN_N_STATES
    for bad in [(grp, hdr + 8, pos, m, fresh, first), (grp, hdr, pos + 4, m, fresh, first), (grp + 2, hdr, pos, m, fresh, first),
                (grp, hdr, pos, m, fresh, first + 1), (grp, hdr + 1, hdr, m, hdr, hdr)]:
        assert ok(*bad) == L.CWH_SEEN_ALIGN, bad
    for bad in [(grp, hdr, pos, m, hdr, first), (grp, hdr, pos, m, hdr + 16 * m - 1, first), (grp, hdr, pos, m, fresh, hdr + 16), (grp, hdr, pos, m, pos + 5, first),
                (grp, hdr, pos, m, fresh, pos + 16 * m - 4), (grp, hdr, pos, m, grp + 3, first), (grp, hdr, pos, m, fresh, grp), (grp, hdr, pos, m, fresh, fresh),
                (grp, hdr, pos, m, first + 4 * m - 1, first), (grp, hdr, pos, m, fresh, fresh + m - 4)]:
        assert ok(*bad) == L.CWH_SEEN_OVERLAP, bad
    assert ok(grp, hdr, pos, m, hdr - m, first) == L.CWH_SEEN_OK and ok(grp, hdr, pos, m, fresh, first + 4 * m) == L.CWH_SEEN_OK      # touching is not sharing
    assert ok(0, hdr, pos, m, 3, first) == L.CWH_SEEN_OK                                        # without a group nothing overlaps address 0
    assert ok(grp, hdr, pos, 0, hdr, hdr) == L.CWH_SEEN_OK                                      # no rows: no bytes to share


def test_seen_slots_of(lib):
    L, h = lib
    assert [h.cwh_seen_slots_of(c) for c in (0, 1, 2, 3, 4, 5, 16, 1000, 1024, 1025)] == [0, 2, 4, 8, 8, 16, 32, 2048, 2048, 4096]
    assert h.cwh_seen_slots_of(L.CWH_SEEN_MAX_CAPACITY) == 2 ** 29 and h.cwh_seen_slots_of(2 ** 27 + 1) == 2 ** 29
    assert h.cwh_seen_slots_of(-1) == -1 and h.cwh_seen_slots_of(L.CWH_SEEN_MAX_CAPACITY + 1) == -1 and h.cwh_seen_slots_of(2 ** 62) == -1
    for c in range(1, 300):
        s = h.cwh_seen_slots_of(c)
        assert s & (s - 1) == 0 and s >= 2 * c and (s // 2 < 2 * c or s == 2)


def _host_keys(h, hdr, pos, group):
    out = np.zeros((len(hdr), KEY_WORDS), np.uint32)
    for j in range(len(hdr)):
        hj, pj = np.ascontiguousarray(hdr[j]), np.ascontiguousarray(pos[j])
        h.cwh_seen_key_of(int(group[j]), hj.ctypes.data, pj.ctypes.data, out[j].ctypes.data)
    return out


def _random_records(n, seed):
    r = np.random.RandomState(seed)
    return r.randint(0, 256, (n, 16)).astype(np.uint8), r.randint(0, 65536, (n, 8)).astype(np.uint16), r.randint(0, 2 ** 31, n).astype(np.int64)


def test_the_host_key_is_the_checkers_key(lib):
    _, h = lib
    hdr, pos, group = _random_records(500, 1)
    assert np.array_equal(_host_keys(h, hdr, pos, group), key_of(hdr, pos, group))
    assert np.array_equal(_host_keys(h, hdr, pos.view(np.int16), group), key_of(hdr, pos.view(np.int16), group))
    odd = np.zeros(16 * 3 + 1, np.uint8)                                                        # any alignment
    odd[1:] = hdr[:3].reshape(-1)
    k = np.zeros(KEY_WORDS, np.uint32)
    h.cwh_seen_key_of(int(group[1]), odd.ctypes.data + 17, np.ascontiguousarray(pos[1]).ctypes.data, k.ctypes.data)
    assert np.array_equal(k, key_of(hdr[1:2], pos[1:2], group[1:2])[0])


def test_excluded_fields_leave_the_key_and_included_bits_change_it(lib):
    _, h = lib
    hdr, pos, group = _random_records(40, 2)
    base = _host_keys(h, hdr, pos, group)
    hashes = lambda k: [h.cwh_seen_hash_of(np.ascontiguousarray(r).ctypes.data) for r in k]  # noqa: E731
    base_hash = hashes(base)
    excluded = [(3, b) for b in range(8)] + [(8, b) for b in range(8)] + [(9, b) for b in range(8)] + [(10, 0)] + [(10, b) for b in range(2, 8)] + \
               [(11, b) for b in range(8)]                                                      # menu, step_num, flag bit 0, the success count
    included = [(byte, b) for byte in (0, 1, 2, 4, 5, 6, 7, 12, 13, 14, 15) for b in range(8)] + [(10, 1)]
    assert len(excluded) + len(included) == 128
    for byte, bit in excluded:
        x = hdr.copy()
        x[:, byte] ^= 1 << bit
        assert np.array_equal(_host_keys(h, x, pos, group), base) and np.array_equal(key_of(x, pos, group), base), (byte, bit)
    for byte, bit in included:
        x = hdr.copy()
        x[:, byte] ^= 1 << bit
        k = _host_keys(h, x, pos, group)
        assert (k != base).any(axis=1).all() and np.array_equal(key_of(x, pos, group), k), (byte, bit)
        assert all(a != b for a, b in zip(hashes(k), base_hash)), (byte, bit)
    for slot in range(8):
        for bit in range(16):
            x = pos.copy()
            x[:, slot] ^= 1 << bit
            k = _host_keys(h, hdr, x, group)
            assert (k != base).any(axis=1).all() and np.array_equal(key_of(hdr, x, group), k), (slot, bit)
    for bit in range(31):
        k = _host_keys(h, hdr, pos, group ^ (1 << bit))
        assert (k != base).any(axis=1).all() and np.array_equal(key_of(hdr, pos, group ^ (1 << bit)), k), bit
    assert len(set(base_hash)) == len(base_hash)


def test_seen_out_mirror_matches_the_header_and_the_abi_names_the_calls(lib, tmp_path):
    L, h = lib
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "craftingworld.h"', 'int main(void){', 'printf("size %zu\\n", sizeof(cw_seen_out));']
    for f, _ in L.cw_seen_out._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(cw_seen_out, %s));' % (f, f))
    lines.append('return 0;}')
    src, exe = tmp_path / 'seen.c', tmp_path / 'seen'
    src.write_text('\n'.join(lines))
    subprocess.check_call(['gcc', '-std=c99', '-pedantic', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got['size']) == C.sizeof(L.cw_seen_out)
    for f, _ in L.cw_seen_out._fields_:
        assert int(got[f]) == getattr(L.cw_seen_out, f).offset
    if not os.environ.get('CW_HOST_LIB'):
        for name in ('cw_seen_reserve', 'cw_seen_clear', 'cw_seen_insert', 'cw_seen_counters', 'cw_seen_slots'):
            assert name in L.ABI and hasattr(h, name), name
        from gym_craftingworld_amd.vec_env import SEEN_FIELDS
        assert SEEN_FIELDS == tuple(f for f, _ in L.cw_seen_out._fields_)


def test_the_epoch_constants_are_the_headers(lib, tmp_path):
    """CWH_SEEN_ROW_BITS and CWH_SEEN_MAX_EPOCH of the binding against cw_host.h as the C++ compiler reads it, what they promise -- the last usable epoch's
    bid epoch << ROW_BITS | row fills the owner word and stays below the empty owner, all ones; MAX_EPOCH + 1, the spent epoch, still fits the shifted field --
    and the epoch's place in the control block (cw_layout.h), which tests/test_seen.py writes"""
    L, _ = lib
    csrc = os.path.join(ROOT, 'gym_craftingworld_amd', 'csrc')
    src, exe = tmp_path / 'epoch.cpp', tmp_path / 'epoch'
    src.write_text('#include <cstdio>\n#include "cw_host.h"\nint main() { printf("%d %llu %lld\\n", CWH_SEEN_ROW_BITS, (unsigned long long)CWH_SEEN_MAX_EPOCH,'
                   ' (long long)CWH_MAX_STATES); return 0; }\n')
    subprocess.check_call(['g++', '-std=c++17', '-Wall', '-Werror', '-I', csrc, str(src), '-o', str(exe)])
    bits, top, rows = (int(x) for x in subprocess.check_output([str(exe)]).decode().split())
    assert (bits, top, rows) == (L.CWH_SEEN_ROW_BITS, L.CWH_SEEN_MAX_EPOCH, L.CWH_MAX_STATES)
    assert rows <= 1 << bits and top + 1 < 1 << (64 - bits)
    assert ((top << bits) | ((1 << bits) - 1)) < 2 ** 64 - 1 and ((top + 1) << bits) < 2 ** 64
    layout = open(os.path.join(csrc, 'cw_layout.h')).read()
    assert 'CW_SEEN_SIZE = 0, CW_SEEN_OVERFLOW = 1, CW_SEEN_COLLISIONS = 2, CW_SEEN_EPOCH = 3, CW_SEEN_TICKET = 4' in layout
    assert '#define CW_SEEN_CTL_WORDS 8\n' in layout


_ASAN_MAIN = r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "cw_host.h"
int main()
{
    // exactly-sized heap records: a read past hdr[16] / slot_pos[8] or a write past key[9] is an ASAN report
    unsigned long long sum = 0;
    for (int j = 0; j < 2000; j++) {
        std::vector<uint8_t> hdr(16);
        std::vector<uint16_t> pos(8);
        std::vector<uint32_t> key(CWH_SEEN_KEY_WORDS);
        for (auto &b : hdr) b = (uint8_t)rand();
        for (auto &p : pos) p = (uint16_t)rand();
        cwh_seen_key_of(j - 5, hdr.data(), pos.data(), key.data());
        const uint64_t h = cwh_seen_hash_of(key.data());
        for (int bits = 0; bits < 64; bits++) if (cwh_seen_tag(h, bits) == 0) return 2;
        sum += h;
    }
    const int64_t caps[] = {-1, 0, 1, 3, 1000, CWH_SEEN_MAX_CAPACITY, CWH_SEEN_MAX_CAPACITY + 1, INT64_MAX};
    for (int64_t c : caps) sum += (unsigned long long)cwh_seen_slots_of(c);
    const uint64_t at[] = {0, 3, 16, 1ull << 20, (1ull << 20) + 4, UINT64_MAX - 15, UINT64_MAX};
    const int32_t ns[] = {INT32_MIN, -1, 0, 1, 100, CWH_MAX_STATES, INT32_MAX};
    for (uint64_t g : at) for (uint64_t h : at) for (uint64_t p : at) for (int32_t n : ns) for (uint64_t f : at) for (uint64_t i : at)
        sum += (unsigned long long)cwh_seen_args(g, h, p, n, f, i);
    if (cwh_seen_args(0, 1ull << 20, 1ull << 21, CWH_MAX_STATES, UINT64_MAX - 15, 0) != CWH_SEEN_OK) return 3;      // a range that would wrap ends at the top
    printf("ok %llu\n", sum);
    return 0;
}
'''


def test_the_host_side_under_asan_and_ubsan(tmp_path):
    """cw_host.cpp and a stand-alone program that drives the cwh_seen_* functions, both built with -fsanitize=address,undefined: exact-size heap
    records, every tag width, the size rule at its edges and the argument rules over addresses at both ends of the address space"""
    csrc = os.path.join(ROOT, 'gym_craftingworld_amd', 'csrc')
    src, exe = tmp_path / 'seen_main.cpp', tmp_path / 'seen_main'
    src.write_text(_ASAN_MAIN)
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                           '-fno-omit-frame-pointer', '-I', csrc, str(src), os.path.join(csrc, 'cw_host.cpp'), '-o', str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0'), timeout=120)
    assert p.returncode == 0 and p.stdout.startswith('ok '), (p.returncode, p.stdout[-500:], p.stderr[-3000:])
    assert 'runtime error' not in p.stderr and 'AddressSanitizer' not in p.stderr, p.stderr[-3000:]
