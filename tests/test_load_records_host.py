"""CPU tier of cw_load_records: the rule a record passes before an env takes it (csrc/cw_host.h: cwh_record_ok, the code the kernel runs) against the
records of oracle walks, the painted states, the boundary cells and every single mutation of a good record; the index check; the argument rules
(cwh_load_records_args); and that the entry point is declared, bound and exported."""
import ctypes as C
import os

import numpy as np
import pytest

from hostlib import host_lib
from load_records_check import MUTATIONS, WALK_ENVS, WALK_SIZES, WALK_STEPS, good_record, mutated, record_rule, walk_records
from records_check import POS_GONE, POS_HELD, encode
from state_tables import painted_states

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ok(lib, S, hdr, pos):
    hdr, pos = np.ascontiguousarray(hdr, dtype=np.uint8), np.ascontiguousarray(pos, dtype=np.uint16)
    return lib.cwh_record_ok_of(S, hdr.ctypes.data, pos.ctypes.data) != 0


@pytest.mark.parametrize('S', WALK_SIZES)
def test_every_record_of_an_oracle_walk_is_accepted(S):
    """12 envs x 400 random steps with auto-reset, encoded after every step: none is refused, and the walk holds what the rule has branches for"""
    _, lib = host_lib()
    hdr, pos = walk_records(S)
    assert len(hdr) == WALK_ENVS * WALK_STEPS
    refused = [j for j in range(len(hdr)) if not _ok(lib, S, hdr[j], pos[j])]
    assert not refused, (len(refused), hdr[refused[0]].tolist(), pos[refused[0]].tolist())
    assert all(record_rule(S, hdr[j], pos[j]) for j in range(0, len(hdr), 7))             # (the rule written from the header's text agrees)
    assert (hdr[:, 2] != 0).sum() > 0 and (pos == POS_HELD).any(axis=1).sum() == (hdr[:, 2] != 0).sum()
    assert (pos == POS_GONE).any(axis=1).sum() > 0                                             # an object gone for good


def test_every_painted_state_is_accepted():
    _, lib = host_lib()
    ps = painted_states(8)
    z = np.zeros(len(ps), np.int64)
    hdr, pos = encode(dict(grid=np.stack([p[1] for p in ps]), agent=np.array([p[3] for p in ps]), hold=np.array([p[4] for p in ps]), achieved=z,
                           desired=z + 5, step_num=z + 2, flags=z + 1))
    for j, p in enumerate(ps):
        assert _ok(lib, 8, hdr[j], pos[j]) and record_rule(8, hdr[j], pos[j]), p[0]


@pytest.mark.parametrize('S', [4, 255])
def test_the_boundary_cell_is_accepted_and_the_next_one_refused(S):
    _, lib = host_lib()
    hdr, pos = good_record(S, last_cell=True)
    assert pos[2] == S * S - 1 and _ok(lib, S, hdr, pos) and record_rule(S, hdr, pos)
    hdr[0], hdr[1] = S - 1, S - 1                               # the agent in the last cell too
    assert _ok(lib, S, hdr, pos)
    pos[2] = S * S
    assert not _ok(lib, S, hdr, pos) and not record_rule(S, hdr, pos)


@pytest.mark.parametrize('S', [4, 5, 21, 255])
@pytest.mark.parametrize('name', MUTATIONS)
def test_every_single_mutation_of_a_good_record_is_refused(name, S):
    _, lib = host_lib()
    hdr, pos = good_record(S)
    assert _ok(lib, S, hdr, pos) and record_rule(S, hdr, pos)
    bad_h, bad_p = mutated(name, S)
    assert not (np.array_equal(bad_h, hdr) and np.array_equal(bad_p, pos))
    assert not _ok(lib, S, bad_h, bad_p), name
    assert not record_rule(S, bad_h, bad_p), name


def test_what_the_rule_leaves_free():
    """the masks, step_num, the flag word and the menu byte take any value"""
    _, lib = host_lib()
    hdr, pos = good_record(5)
    hdr[3] = 255
    hdr[4:12] = 255
    assert _ok(lib, 5, hdr, pos) and record_rule(5, hdr, pos)
    hdr[4:12] = 0
    assert _ok(lib, 5, hdr, pos)
    hdr[2], pos[1] = 0, POS_GONE                                 # nothing held, the axe gone: its code must go too
    assert not _ok(lib, 5, hdr, pos)
    hdr[12] &= 0x0F
    assert _ok(lib, 5, hdr, pos) and record_rule(5, hdr, pos)


def test_the_library_and_the_written_rule_agree_on_random_records():
    """records drawn near the rule's edges: the two implementations give the same verdict on each, and both verdicts occur"""
    _, lib = host_lib()
    rs = np.random.RandomState(3)
    S, seen = 4, [0, 0]
    for _ in range(4000):
        hdr, pos = good_record(S)
        for _ in range(rs.randint(0, 3)):
            k = rs.randint(8)
            what = rs.randint(4)
            if what == 0:
                pos[k] = rs.choice([POS_GONE, POS_HELD, 0xFFFD, S * S, rs.randint(S * S)])
            elif what == 1:
                hdr[12 + k // 2] = rs.randint(256)
            elif what == 2:
                hdr[rs.randint(3)] = rs.choice([0, 1, 2, 3, 4, S, 255])
            else:
                hdr[4 + rs.randint(8)] = rs.randint(256)
        got = _ok(lib, S, hdr, pos)
        assert got == record_rule(S, hdr, pos), (hdr.tolist(), pos.tolist())
        seen[int(got)] += 1
    assert min(seen) > 400, seen


def test_an_index_becomes_an_address_only_inside_the_records():
    _, lib = host_lib()
    f = lib.cwh_load_record_index_in_range
    assert [f(i, 5) for i in (-(2 ** 31), -7, -1, 0, 4, 5, 6, 2 ** 31 - 1)] == [0, 0, 0, 1, 1, 0, 0, 0]
    assert f(0, 0) == 0 and f(2 ** 27 - 1, 2 ** 27) == 1


def test_the_argument_rules():
    L, lib = host_lib()
    N, A = 70, 1 << 20                                          # (addresses as integers: nothing is dereferenced)
    eh, ep = 1 << 40, (1 << 40) + 16 * N

    def rc(src=A, hdr=2 * A, pos=3 * A, n=40, status=4 * A):
        return lib.cwh_load_records_args(N, src, hdr, pos, n, status, eh, ep)
    assert rc() == L.CWH_LOAD_OK and rc(status=0) == L.CWH_LOAD_OK and rc(n=0) == L.CWH_LOAD_OK
    assert rc(hdr=0) == rc(pos=0) == L.CWH_LOAD_NO_RECORDS
    assert rc(n=-1) == rc(n=2 ** 27 + 1) == L.CWH_LOAD_N_RECORDS and rc(n=2 ** 27, status=0) == L.CWH_LOAD_OK
    assert rc(src=0, n=N) == L.CWH_LOAD_OK and rc(src=0, n=N - 1) == rc(src=0, n=N + 1) == rc(src=0, n=0) == L.CWH_LOAD_OWN_ORDER
    assert rc(hdr=2 * A + 8) == rc(pos=3 * A + 4) == rc(src=A + 2) == L.CWH_LOAD_ALIGN and rc(src=A + 4) == L.CWH_LOAD_OK
    # the records and the engine's own buffers: a shared byte at either end, either array, either buffer
    assert rc(hdr=eh) == rc(pos=eh) == rc(hdr=ep) == rc(pos=ep) == L.CWH_LOAD_ENGINE_OVERLAP
    assert rc(hdr=eh - 16 * 40 + 16) == rc(pos=ep + 16 * N - 16) == L.CWH_LOAD_ENGINE_OVERLAP
    assert rc(hdr=eh - 16 * 40) == rc(pos=ep + 16 * N) == L.CWH_LOAD_OK
    assert rc(hdr=eh, n=0) == L.CWH_LOAD_OK                      # (no record: no byte shared)
    # status and what the kernel reads
    assert rc(status=2 * A) == rc(status=2 * A + 16 * 40 - 1) == rc(status=3 * A - N + 1) == rc(status=A) == rc(status=A + 4 * N - 1) == L.CWH_LOAD_STATUS_OVERLAP
    assert rc(status=2 * A + 16 * 40) == rc(status=A + 4 * N) == rc(status=A - N) == L.CWH_LOAD_OK
    assert rc(src=0, n=N, status=2 * A + 16 * N - 1) == L.CWH_LOAD_STATUS_OVERLAP


def test_the_entry_point_is_declared_bound_and_exported():
    L, lib = host_lib()
    header = open(os.path.join(ROOT, 'include', 'craftingworld.h')).read()
    assert 'int cw_load_records(cw_engine *e, const int32_t *src, const uint8_t *hdr, const uint16_t *slot_pos, int32_t n_records, uint8_t *status,' in header
    assert 'then cw_load_records' in header.split('#define CW_ABI_VERSION')[1].split('*/')[0] and L.CW_ABI_VERSION == 5
    assert 'envs a snapshot or record load skipped' in header
    for name in ('cwh_record_ok_of', 'cwh_load_record_index_in_range', 'cwh_load_records_args'):
        assert name in L.HOST_HELPERS and getattr(lib, name).restype is C.c_int
    if not os.environ.get('CW_HOST_LIB'):                       # (the sanitizer build holds cw_host.cpp alone)
        fn = lib.cw_load_records
        assert fn.restype is C.c_int and len(fn.argtypes) == 7
        from gym_craftingworld_amd import CraftingWorldVecEnv, vec_env
        assert callable(CraftingWorldVecEnv.load_records) and callable(vec_env.load_records_args) and callable(vec_env.load_records_src)
        assert 'load_records' in CraftingWorldVecEnv.snapshot_skipped.__doc__
