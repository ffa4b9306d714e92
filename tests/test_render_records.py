"""GPU tier of render_records: cw_render_records_kernel through CraftingWorldVecEnv.render_records and, for the call order and the argument errors, through
ctypes.  Frames are compared with the CPU oracle's rasterisers of hand-built or decoded states and with the engine's own render() / observation array;
where an output array is a view into a sentinel-filled buffer the whole buffer is checked with render_records_check.check_frames (itself tested on the CPU,
tests/test_render_records_logic.py).  Only possible records are fed (impossible ones: tests/test_render_records_host.py, through the offset helper alone).
Everything is bit-exact.  No timing."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from engines import K5, n_cu
from masked_check import spread, take
from oracle_replay import make_env, np_states
from records_check import decode
from render_records_check import check_frames, dense_of, frame_bytes, frame_shape, oracle_frames, records_launch, records_of
from state_tables import painted_states

pytestmark = pytest.mark.gpu

SENT = 0xA5
RASTERS = ['ray', 'alt']


def _engine(S, raster, N=2, **kw):
    from gym_craftingworld_amd import CraftingWorldVecEnv
    env = CraftingWorldVecEnv(N, **dict(dict(size=(S, S), max_steps=17, obs_mode='state', raster=raster, seed=11), **kw))
    env.reset()
    return env


@functools.lru_cache(maxsize=None)
def _painted(S, alt):
    """painted_states(S) as records and the oracle's frame of each, computed once -> (hdr [n, 16], slot_pos [n, 8], frames [n, ...], the states)"""
    ps = painted_states(S)
    hdr, pos = records_of(ps)
    d = dense_of(ps)
    want = oracle_frames(d['grid'], d['agent'], d['hold'], alt)
    return hdr, pos, want, ps


def _buffer(M, fb, lo, pad=64):
    """a sentinel-filled device buffer whose base is 16-byte aligned, and the [M, fb] view of it that starts `lo` bytes in"""
    buf = torch.full((lo + M * fb + pad,), SENT, dtype=torch.uint8, device='cuda')
    assert buf.data_ptr() % 16 == 0
    return buf, buf[lo:lo + M * fb]


def _same_frames(got, want, tag):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint8, (tag, got.shape, got.dtype, want.shape, want.dtype)
    bad = np.flatnonzero((got != want).reshape(len(want), -1).any(axis=1))
    assert len(bad) == 0, '%s: frames of %d states differ, first %s' % (tag, len(bad), bad[:8].tolist())


# ------------------------------------------------------------------------------------------------------------------------------ 1. against the oracle
@pytest.mark.parametrize('raster', RASTERS)
@pytest.mark.parametrize('S', [5, 8, 21, 255])
def test_hand_built_states_against_the_oracle(S, raster):
    """the state classes a painter can get wrong, packed into records on the host, at every size class (255: slot positions above 32 767, frames of megabytes);
    what the table holds is counted from the table alone, before anything is compared"""
    alt = raster == 'alt'
    hdr, pos, want, ps = _painted(S, alt)
    holds = {p[4] for p in ps}
    agents = {p[3] for p in ps}
    assert holds == {0, 1, 2, 3}
    assert {(0, 0), (0, S - 1), (S - 1, 0), (S - 1, S - 1)} <= agents
    assert any(p[1][0, 0] != 0 for p in ps) and any(p[1][S - 1, S - 1] != 0 for p in ps)
    assert any(p[4] == 1 and p[1][p[3]] == 1 for p in ps)                              # sticks held over a sticks cell
    env = _engine(S, raster)
    f = env.render_records(hdr, pos)
    assert f.dtype == torch.uint8 and tuple(f.shape) == (len(ps),) + frame_shape(S, alt) == (len(ps),) + tuple(env.frame_shape) and f.is_cuda
    _same_frames(f.cpu().numpy(), want, 'S = %d' % S)
    f2 = env.render_records(torch.as_tensor(hdr.copy(), device='cuda'), torch.as_tensor(pos.copy(), device='cuda'))          # (device records go over in place)
    assert torch.equal(f, f2)
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 2. against the engine itself
@pytest.mark.parametrize('obs_mode', ['state', 'pixels_dirty', 'pixels'])
@pytest.mark.parametrize('raster', RASTERS)
@pytest.mark.parametrize('S', [4, 5, 21])
def test_the_engines_own_records_give_the_engines_own_frames(S, raster, obs_mode):
    """a stepped batch, with and without auto_reset: render_records(env.hdr, env.slot_pos) == render(), and in the pixel modes == the observation array"""
    N = 67
    for auto_reset in (True, False):
        env, _, _ = make_env(N, *np_states(N, 71000 + S), size=(S, S), max_steps=17, obs_mode=obs_mode, raster=raster, auto_reset=auto_reset)
        env.reset()
        spread(env, 2 * 17 + 3, 5 + S)
        f = env.render_records(env.hdr, env.slot_pos)
        want = env.render()
        assert f.dtype == want.dtype == torch.uint8 and f.shape == want.shape
        tag = 'S = %d %s %s auto_reset=%s' % (S, raster, obs_mode, auto_reset)
        _same_frames(f.cpu().numpy(), want.cpu().numpy(), tag + ': render()')
        if obs_mode != 'state':
            _same_frames(f.cpu().numpy(), env._observation()['observation'].cpu().numpy(), tag + ': observation')
        assert len(np.unique(f.cpu().numpy().reshape(N, -1), axis=0)) > N // 2, tag       # (the batch is not all alike)
        env.close()


@pytest.mark.parametrize('raster', RASTERS)
def test_a_host_outputs_engine_of_one_env(raster):
    from gym_craftingworld_amd import CraftingWorldVecEnv
    env = CraftingWorldVecEnv(1, size=(5, 5), max_steps=17, obs_mode='pixels', raster=raster, host_outputs=True, seed=4)
    env.reset()
    acts = np.random.RandomState(3).randint(0, 6, 23)
    for t in range(len(acts)):
        obs, _, _, _ = env.step(acts[t:t + 1])
        f = env.render_records(env.hdr, env.slot_pos)
        _same_frames(f.cpu().numpy(), np.asarray(obs['observation'].cpu().numpy()), 'step %d: observation' % t)
    _same_frames(env.render_records(env.hdr, env.slot_pos).cpu().numpy(), env.render().cpu().numpy(), 'render()')
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 3. launch shapes
@pytest.mark.parametrize('raster', RASTERS)
def test_launch_shapes(raster):
    """M = 1, one wave's worth and one more or less, and more states than the launch has waves (the grid-stride loop's second trip): every frame is its
    source state's"""
    alt = raster == 'alt'
    hdr, pos, want, ps = _painted(5, alt)
    cus = n_cu()
    big = 4 * cus + 5
    assert records_launch(big, cus) == 4 * cus < big and records_launch(65, cus) == 68
    env = _engine(5, raster)
    for M in (1, 63, 64, 65, big):
        src = np.arange(M) % len(ps)
        buf, out = _buffer(M, want[0].nbytes, 16)
        f = env.render_records(hdr[src], pos[src], out=out.view((M,) + want.shape[1:]))
        assert f.data_ptr() == out.data_ptr()
        assert len(check_frames(buf.cpu().numpy(), 16, want[src], None, SENT)) == M
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 4. mask and guards
def _masks(M):
    last = np.zeros(M, np.uint8)
    last[-1] = 1
    return {'all': np.ones(M, np.uint8), 'none': np.zeros(M, np.uint8), 'alternating': (np.arange(M) % 2 * 255).astype(np.uint8), 'last': last}


@pytest.mark.parametrize('raster', RASTERS)
def test_mask_and_guard_bytes(raster):
    """out is a view into a sentinel-filled buffer, at every byte offset from a 16-byte boundary (AltObs) or every multiple of 4 (Ray): masked-out frames and
    the bytes around the array keep the sentinel, for masks all / none / alternating / only the last row, as uint8 and as bool"""
    alt = raster == 'alt'
    hdr, pos, want, ps = _painted(5, alt)
    M, fb = 37, frame_bytes(5, alt)
    src = np.arange(M) % len(ps)
    env = _engine(5, raster)
    h, p = torch.as_tensor(hdr[src], device='cuda'), torch.as_tensor(pos[src], device='cuda')
    for lo in (range(16) if alt else (0, 4, 8, 12)):
        for name, m in _masks(M).items():
            buf, out = _buffer(M, fb, 16 + lo)
            assert out.data_ptr() % 16 == lo
            mask = torch.as_tensor(m, device='cuda')
            mask = (mask != 0) if lo % 2 else mask                                      # (bool and uint8 masks, device tensors both: in place)
            env.render_records(h, p, mask=mask, out=out.view((M,) + want.shape[1:]))
            rows = check_frames(buf.cpu().numpy(), 16 + lo, want[src], m, SENT, allow_empty=name == 'none')
            assert len(rows) == {'all': M, 'none': 0, 'alternating': M // 2, 'last': 1}[name], (lo, name)
    buf, out = _buffer(M, fb, 16)                                                       # a mask from the host, and none at all
    env.render_records(h, p, mask=_masks(M)['alternating'] != 0, out=out.view((M,) + want.shape[1:]))
    check_frames(buf.cpu().numpy(), 16, want[src], _masks(M)['alternating'], SENT)
    if not alt:                                                                         # the Ray painter's 12-byte stores need a 4-byte aligned array
        buf, out = _buffer(M, fb, 16 + 2)
        with pytest.raises(ValueError, match='4-byte aligned'):
            env.render_records(h, p, out=out.view((M,) + want.shape[1:]))
        torch.cuda.synchronize()
        assert bool((buf == SENT).all())                                                # (nothing enqueued)
    with pytest.raises(ValueError):
        env.render_records(h, p, mask=torch.ones(M + 1, dtype=torch.uint8, device='cuda'))
    with pytest.raises(ValueError):
        env.render_records(h, p, mask=torch.ones(M, dtype=torch.int32, device='cuda'))
    with pytest.raises(ValueError):
        env.render_records(h, p, out=torch.empty((M,) + want.shape[1:], dtype=torch.int16, device='cuda'))
    with pytest.raises(ValueError):
        env.render_records(h, p, out=torch.empty((M + 1,) + want.shape[1:], dtype=torch.uint8, device='cuda'))
    with pytest.raises(ValueError):
        env.render_records(h, p, out=torch.empty((M,) + want.shape[1:], dtype=torch.uint8))
    with pytest.raises(ValueError):
        env.render_records(h, p, out=torch.empty((M, 2) + want.shape[1:], dtype=torch.uint8, device='cuda')[:, 0])
    empty = env.render_records(h[:0], p[:0])
    assert tuple(empty.shape) == (0,) + want.shape[1:]
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 5. purity
@pytest.mark.parametrize('raster', RASTERS)
def test_nothing_of_the_engine_is_written(raster):
    """an auto-reset engine that keeps look-ahead records and frames: everything take() reads -- states, streams, buffers, counters, the three frame arrays --
    is byte-identical before and after the calls"""
    N = 70
    env, _, _ = make_env(N, *np_states(N, 72000), obs_mode='pixels_dirty', raster=raster, **K5)
    assert env.tuner_state()['lookahead'] == 1
    env.reset()
    spread(env, 2 * 17 + 3, 8)
    r = env.expand()
    torch.cuda.synchronize()
    before = take(env)
    env.render_records(env.hdr, env.slot_pos)
    env.render_records(r['hdr'], r['slot_pos'], mask=r['changed'])
    env.render_records(r['hdr'].cpu().numpy(), r['slot_pos'].cpu().numpy(), mask=np.arange(6 * N).reshape(6, N) % 3 == 0)
    torch.cuda.synchronize()
    after = take(env)
    assert set(before) == set(after)
    for k in sorted(before):
        assert np.array_equal(before[k], after[k]), k
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 6. with its siblings
@pytest.mark.parametrize('raster', RASTERS)
def test_frames_of_expand_and_simulate_records(raster):
    """expand()'s successors with mask = changed: every changed successor's frame is the oracle's frame of the DECODED successor, every unchanged row keeps
    the sentinel; the same for simulate()'s final records"""
    alt, S, N = raster == 'alt', 5, 90
    env, _, _ = make_env(N, *np_states(N, 73000), obs_mode='state', raster=raster, **K5)
    env.reset()
    spread(env, 9, 12)
    fb = frame_bytes(S, alt)
    r = env.expand()
    buf, out = _buffer(6 * N, fb, 16)
    f = env.render_records(r['hdr'], r['slot_pos'], mask=r['changed'], out=out.view((6, N) + frame_shape(S, alt)))
    assert tuple(f.shape) == (6, N) + frame_shape(S, alt)
    d = decode(r['hdr'].cpu().numpy().reshape(-1, 16), r['slot_pos'].cpu().numpy().reshape(-1, 8), S)
    changed = r['changed'].cpu().numpy().reshape(-1)
    assert 100 <= changed.sum() <= 6 * N - 100 and (d['hold'][changed] != 0).any()
    want = oracle_frames(d['grid'], d['agent'], d['hold'], alt)
    assert len(check_frames(buf.cpu().numpy(), 16, want, changed, SENT)) == changed.sum()
    T, K = 6, 3
    gen = torch.Generator(device='cuda').manual_seed(4)
    acts = torch.randint(0, 6, (T, K * N), device='cuda', dtype=torch.uint8, generator=gen)
    s = env.simulate(acts)
    buf, out = _buffer(K * N, fb, 16)
    env.render_records(s['hdr'], s['slot_pos'], out=out.view((K * N,) + frame_shape(S, alt)))
    d = decode(s['hdr'].cpu().numpy(), s['slot_pos'].cpu().numpy(), S)
    want = oracle_frames(d['grid'], d['agent'], d['hold'], alt)
    assert len(np.unique(want.reshape(K * N, -1), axis=0)) > N // 2
    check_frames(buf.cpu().numpy(), 16, want, None, SENT)
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 7. graph capture
@pytest.mark.parametrize('raster', RASTERS)
def test_captured_into_a_graph_with_expand(raster):
    """expand(out=...) + render_records(mask=changed, out=...) in one torch.cuda.graph on one stream: capturing runs nothing; replayed after the env has
    stepped, the frames are those of an eager call on the new states"""
    alt, S, N = raster == 'alt', 5, 150
    env, _, _ = make_env(N, *np_states(N, 74000), obs_mode='state', raster=raster, **K5)
    env.reset()
    spread(env, 5, 6)
    r = env.expand()
    frames = torch.full((6, N) + frame_shape(S, alt), SENT, dtype=torch.uint8, device='cuda')
    env.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.expand(out=r)
        env.render_records(r['hdr'], r['slot_pos'], mask=r['changed'], out=frames)
    assert bool((frames == SENT).all())                                                 # (capturing ran nothing)
    seen = []
    for rnd in range(2):
        spread(env, 3, 7 + rnd)
        frames.fill_(SENT)
        g.replay()
        e = env.expand()
        eager = env.render_records(e['hdr'], e['slot_pos'], mask=e['changed'], out=torch.full_like(frames, SENT))
        assert torch.equal(r['hdr'], e['hdr']) and torch.equal(frames, eager), rnd
        assert bool((frames != SENT).any())
        seen.append(frames.clone())
    assert not torch.equal(seen[0], seen[1])
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 8. past 4 GiB
def test_an_output_array_past_4_gib():
    """21 x 21 Ray, 16 records tiled to M = 202 904 states, an array that passes 2^32 bytes: frame j equals frame j % 16 for every j, compared on the device, and
    the first and the last 16 frames equal the oracle's"""
    hdr, pos, want, ps = _painted(21, False)
    fb = frame_bytes(21, False)
    M = 202904                                                                          # (2^32 bytes end inside frame 202 899: the last five frames lie past them)
    assert (M - 5) * fb < 2 ** 32 < (M - 4) * fb
    if torch.cuda.mem_get_info()[0] < 3 * M * fb:
        pytest.skip('needs %.1f GB of free device memory' % (3 * M * fb / 1e9))
    env = _engine(21, 'ray')
    src = torch.arange(M, device='cuda') % 16
    h, p = torch.as_tensor(hdr[:16].copy(), device='cuda')[src], torch.as_tensor(pos[:16].copy(), device='cuda')[src]
    f = env.render_records(h, p).view(M, fb)
    whole = M // 16
    assert bool((f[:whole * 16].view(whole, 16, fb) == f[:16]).all()) and torch.equal(f[whole * 16:], f[:M - whole * 16])
    _same_frames(f[:16].cpu().numpy().reshape(want[:16].shape), want[:16], 'the first 16 frames')
    tail = (np.arange(M - 16, M) % 16)
    _same_frames(f[M - 16:].cpu().numpy().reshape(want[:16].shape), want[tail], 'the last 16 frames')
    del f
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 9. call order and arguments through ctypes
@pytest.mark.parametrize('raster', RASTERS)
def test_call_order_and_arguments_through_ctypes(raster):
    from gym_craftingworld_amd import CraftingWorldVecEnv, _lib as L
    alt, N = raster == 'alt', 8
    env = CraftingWorldVecEnv(N, obs_mode='state', auto_reset=False, raster=raster, seed=3, **K5)
    lib, h, st = env._lib, env._h, env._stream()
    fb = frame_bytes(5, alt)
    vp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    buf = torch.full((N * fb + 64,), SENT, dtype=torch.uint8, device='cuda')
    mask = torch.ones(N, dtype=torch.uint8, device='cuda')
    assert lib.cw_render_records(h, vp(env.hdr), vp(env.slot_pos), None, N, vp(buf), st) == L.CW_ERR_STATE and b'before cw_reset' in lib.cw_last_error()
    env.reset()
    hdr, pos, out = vp(env.hdr), vp(env.slot_pos), vp(buf)
    invalid = [((None, hdr, pos, None, N, out), b'null engine'), ((h, None, pos, None, N, out), b'null hdr'), ((h, hdr, None, None, N, out), b'null slot_pos'),
               ((h, hdr, pos, None, N, None), b'null out_frames'),
               ((h, hdr, pos, None, -1, out), b'n_states'), ((h, hdr, pos, None, 2 ** 27 + 1, out), b'n_states'),
               ((h, vp(env.hdr, 8), pos, None, N - 1, out), b'hdr is not 16-byte aligned'),
               ((h, hdr, vp(env.slot_pos, 2), None, N - 1, out), b'slot_pos is not 16-byte aligned'),
               ((h, hdr, pos, None, N, hdr), b'overlaps the records'),
               ((h, hdr, pos, None, N, vp(env.hdr, 16 * N - 4)), b'overlaps the records'),
               ((h, hdr, pos, None, N, pos), b'overlaps the records'),
               ((h, hdr, pos, vp(buf, 12), N, out), b'overlaps the mask')]
    if not alt:
        invalid += [((h, hdr, pos, None, N, vp(buf, 2)), b'out_frames is not 4-byte aligned'), ((h, hdr, pos, None, N, vp(buf, 1)), b'4-byte aligned')]
    for args, word in invalid:
        assert lib.cw_render_records(*args, st) == L.CW_ERR_INVALID, word
        assert word in lib.cw_last_error(), (word, lib.cw_last_error())
    assert lib.cw_render_records(h, hdr, pos, vp(mask), 0, out, st) == L.CW_OK                # no states: nothing enqueued
    torch.cuda.synchronize()
    assert bool((buf == SENT).all())
    assert lib.cw_render_records(h, hdr, pos, vp(mask), N, vp(buf, 32), st) == L.CW_OK
    torch.cuda.synchronize()
    want = env.render().cpu().numpy()
    check_frames(buf.cpu().numpy(), 32, want, None, SENT)
    env.close()
