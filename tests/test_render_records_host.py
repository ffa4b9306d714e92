"""CPU tier: the host side of render_records -- the checked pixel offset cw_render_records_kernel's AltObs painter shares with the host (cw_host.h:
cwh_alt_pixel_offset, through its exported twin), vec_env.render_records_args (what cw_render_records is handed, validated without a GPU), and the ABI
entry.  Impossible records -- an item code or a position that is anything -- are covered here, through the helper alone: the GPU tier feeds possible ones."""
import ctypes as C
import os

import numpy as np
import pytest

from hostlib import ROOT, host_lib
from state_tables import oracle_frame

POSITIONS = lambda S: (0, S * S - 1, S * S, 0x7FFF, 0x8000, 0xFFFE, 0xFFFF)  # noqa: E731


@pytest.mark.parametrize('S', [4, 5, 21, 255])
def test_the_pixel_offset_stays_inside_the_frame_for_any_item_and_position(S):
    """S x (the cells at both ends, the first position off the grid, both sides of the sign bit, the two markers) x every item byte 0..255: the result is
    "none" or a pixel inside the grid part of the frame, and "none" for every item outside 1..9 and every position at or above S * S"""
    L, lib = host_lib()
    f, none = lib.cwh_alt_pixel_offset_of, L.CWH_ALT_NO_PIXEL
    frame_bytes = 27 * S * (S + 1)
    some = 0
    for pos in POSITIONS(S):
        for item in range(256):
            off = f(S, pos, item)
            if not (1 <= item <= 9) or pos >= S * S:
                assert off == none, (S, pos, item, off)
            else:
                assert off != none and off % 3 == 0 and off + 3 <= frame_bytes, (S, pos, item, off)
                r, c, k = pos // S, pos % S, item - 1
                assert off == ((3 * r + k // 3) * 3 * S + 3 * c + k % 3) * 3
                some += 1
    assert some == 9 * sum(p < S * S for p in POSITIONS(S)) >= 18
    for size in (0, 256, 65536, 2 ** 32 - 1):                    # (no engine has such a size: nothing is drawn, nothing overflows)
        assert f(size, 0, 1) == none


def test_the_pixel_offset_is_the_pixel_the_oracle_lights():
    """items 1..9 at every cell of a 5 x 5 grid: the offset is the ONE pixel the oracle's AltObs rasteriser lights for that object alone (item 9: the agent)"""
    L, lib = host_lib()
    S = 5
    far = lambda cell: ((cell // S + 2) % S, (cell % S + 2) % S)  # noqa: E731  (an agent's cell away from the object's)
    for cell in range(S * S):
        for item in range(1, 10):
            grid = np.zeros((S, S), np.uint8)
            if item == 9:
                lit = oracle_frame(grid, (cell // S, cell % S), 0, True)
            else:
                agent = far(cell)
                empty = oracle_frame(grid, agent, 0, True)
                grid[cell // S, cell % S] = item
                with_it = oracle_frame(grid, agent, 0, True)
                assert (with_it >= empty).all()
                lit = with_it - empty
            px = np.flatnonzero(lit.reshape(-1, 3).any(axis=1))
            off = lib.cwh_alt_pixel_offset_of(S, cell, item)
            assert len(px) == 1 and off == 3 * int(px[0]), (cell, item, px.tolist(), off)


def test_render_records_args():
    from gym_craftingworld_amd.vec_env import render_records_args
    fs = (18, 15, 3)
    hdr, pos = np.zeros((6, 7, 16), np.uint8), np.zeros((6, 7, 8), np.int16)
    assert render_records_args(fs, hdr, pos) == (42, (6, 7))
    assert render_records_args(fs, hdr, pos.view(np.uint16), mask=np.ones((6, 7), bool), out=np.empty((6, 7) + fs, np.uint8)) == (42, (6, 7))
    assert render_records_args(fs, hdr[0], pos[0], mask=np.ones(7, np.uint8)) == (7, (7,))
    assert render_records_args(fs, hdr[:0], pos[:0], mask=np.ones((0, 7), np.uint8), out=np.empty((0, 7) + fs, np.uint8)) == (0, (0, 7))
    bad = [dict(hdr=None), dict(slot_pos=None),
           dict(hdr=hdr[..., :15]), dict(hdr=hdr.astype(np.int8)), dict(slot_pos=pos[..., :7]), dict(slot_pos=pos.astype(np.int32)),
           dict(hdr=hdr[:5]), dict(slot_pos=pos.reshape(42, 8)),
           dict(mask=np.ones((6, 7), np.int32)), dict(mask=np.ones((6, 7), np.float32)), dict(mask=np.ones((7, 6), bool)), dict(mask=np.ones(42, bool)),
           dict(mask=np.ones((6, 7, 1), np.uint8)),
           dict(out=np.empty((6, 7) + fs, np.int8)), dict(out=np.empty((6, 7) + fs, np.int16)), dict(out=np.empty((42,) + fs, np.uint8)),
           dict(out=np.empty((6, 7, 18, 15), np.uint8)), dict(out=np.empty((6, 7, 20, 20, 3), np.uint8)),
           dict(out=np.empty((6, 7, 18, 15, 6), np.uint8)[..., ::2]), dict(out=[[0]])]
    for kw in bad:
        args = dict(dict(hdr=hdr, slot_pos=pos), **kw)
        with pytest.raises(ValueError):
            render_records_args(fs, **args)
    with pytest.raises(ValueError, match='2\\*\\*27'):
        render_records_args(fs, np.broadcast_to(hdr[0, 0], (2 ** 27 + 1, 16)), np.broadcast_to(pos[0, 0], (2 ** 27 + 1, 8)))


def test_the_abi_entry_and_the_header():
    L, lib = host_lib()
    vp = C.c_void_p
    assert L.ABI['cw_render_records'] == (C.c_int, [vp, vp, vp, vp, C.c_int32, vp, vp])
    assert L.HOST_HELPERS['cwh_alt_pixel_offset_of'] == (C.c_uint32, [C.c_uint32] * 3)
    hdr = open(os.path.join(ROOT, 'include', 'craftingworld.h')).read()
    assert 'int cw_render_records(cw_engine *e, const uint8_t *hdr, const uint16_t *slot_pos, const uint8_t *mask' in hdr
    listed = hdr[hdr.index('added since without a new number'):hdr.index('4: cw_tuner_state')]
    assert 'cw_render_records' in listed
    if not os.environ.get('CW_HOST_LIB'):                        # (the product library: the call is there, and the number stayed)
        assert hasattr(lib, 'cw_render_records') and lib.cw_abi_version() == L.CW_ABI_VERSION == 5
