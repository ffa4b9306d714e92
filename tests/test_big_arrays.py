"""GPU tier of frame arrays and exports PAST 2^32 BYTES.  The sweep (render_pieces, cw_render_gather_kernel) indexes a chunk of a frame array with 32-bit
offsets, and the host rule that keeps every chunk below 2^32 bytes (csrc/cw_host.h: cwh_piece_chunks; tests/test_piece_chunks_host.py) never met frames of
which fewer than 4 096 fill 4 GiB; every other painter and export addresses with size_t and had never been run there.  Here whole arrays of 4.3-4.4 GB: the
sweep over large frames (a) and over many small ones (b), the per-env painters of reset, imagine, snapshot load and the terminal frame at an env offset
past 2^32 (c), and the one-hot and int-image exports (d).  Whole arrays are compared on the device; the envs at the ends of the array, around byte 2^31
and byte 2^32 and at both ends of every chunk of the sweep are compared exactly with frames the CPU oracle's rasterisers paint from get_state().
Every case holds 5-45 GB of device memory and skips only on a card that has less free; it prints its peak and its time (pytest -s)."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import imagine_model as M
from masked_check import model_imagine
from oracle_replay import FRAMES, make_env, one_hot_of, oracle_kw, record_steps, replay_against_oracle, same, same_states, same_terminal

pytestmark = pytest.mark.gpu

SENT = 7                    # a byte no frame holds: not a channel of COLORS_N (ray.py:28-31) or CPV_COLORS (altobs.py:26-27), nor twice one modulo 256
GB = 1e9


def _frame_bytes(S, raster):
    return 27 * S * (S + 1) if raster == 'alt' else 48 * S * S


class _Meter:
    """device memory in use beyond what was in use at the start (the engine's arrays are not torch's: mem_get_info), sampled where the test says, and time"""

    def __init__(self, what, need):
        free, total = torch.cuda.mem_get_info()
        if free < need:
            pytest.skip('%s needs %.1f GB of device memory, %.1f GB are free' % (what, need / GB, free / GB))
        self.what, self.base, self.peak, self.t0 = what, total - free, 0, time.time()

    def tick(self):
        torch.cuda.synchronize()
        free, total = torch.cuda.mem_get_info()
        self.peak = max(self.peak, total - free - self.base)

    def done(self):
        self.tick()
        print('\nbig arrays: %s: peak %.1f GB, %.1f s' % (self.what, self.peak / GB, time.time() - self.t0))
        torch.cuda.empty_cache()


def _chunks(env, FB, rounds=896):
    """(chunks, per) of the sweep over one frame array of this engine: the rule the launcher runs, with the card's CU count"""
    from gym_craftingworld_amd import _lib as L
    per = C.c_int(0)
    n_cu = torch.cuda.get_device_properties(env.device).multi_processor_count
    return L.load().cwh_piece_chunks_of(env.num_envs, FB, n_cu, rounds, C.byref(per)), per.value


def _rows_at(N, unit, chunks=0, per=0):
    """the envs compared with the oracle: both ends of an array of N rows of `unit` bytes, the rows that hold byte 2^31 and byte 2^32 with a neighbour on each
    side, and the first and last env of every chunk of the sweep"""
    rows = {0, N - 1}
    for byte in (2 ** 31, 2 ** 32):
        rows |= {byte // unit - 1, byte // unit, byte // unit + 1}
    for c in range(chunks):
        rows |= {c * per, min(N, (c + 1) * per) - 1}
    return np.array(sorted(r for r in rows if 0 <= r < N))


def _paint(grid, agent, hold, alt):
    """the oracle's rasterisers (cwo_render / cwo_render_alt) on one state"""
    from oracle.oracle import _lib
    u8p = C.POINTER(C.c_uint8)
    g = np.ascontiguousarray(grid, dtype=np.uint8)
    s = g.shape[0]
    out = np.empty((3 * s + 3, 3 * s, 3) if alt else (4 * s, 4 * s, 3), dtype=np.uint8)
    fn = _lib().cwo_render_alt if alt else _lib().cwo_render
    fn.argtypes, fn.restype = [C.c_int32, u8p, C.c_int32, C.c_int32, C.c_int32, u8p], None
    fn(s, g.ctypes.data_as(u8p), int(agent[0]), int(agent[1]), int(hold), out.ctypes.data_as(u8p))
    return out


def _oracle_frames(st, rows, alt):
    """the three frame arrays' rows `rows` as the oracle paints them from get_state(): the current state, the state at reset and the goal state (nothing held)"""
    return {'observation': np.stack([_paint(st['grid'][i], st['agent_rc'][i], st['hold'][i], alt) for i in rows]),
            'init_observation': np.stack([_paint(st['init_grid'][i], st['init_agent_rc'][i], 0, alt) for i in rows]),
            'desired_goal': np.stack([_paint(st['goal_grid'][i], st['goal_agent_rc'][i], 0, alt) for i in rows])}


def _dev(env, rows):
    return torch.as_tensor(np.asarray(rows, dtype=np.int64), device=env.device)


def _check_frame_arrays(env, rows, meter, tag, after_reset):
    """the three assertions of a frame array past 2^32 bytes: the whole observation array == render() (cw_render_frames_kernel) on the device (and, right after
    a reset, init_observation == observation); rows `rows` of all three == the oracle's rasteriser on get_state(); no sentinel byte left anywhere"""
    obs = env._observation()
    shown = env.render()
    meter.tick()
    assert torch.equal(obs['observation'], shown), tag + ': observation != render()'
    del shown
    if after_reset:
        assert torch.equal(obs['init_observation'], obs['observation']), tag + ': init_observation != observation'
    meter.tick()
    want = _oracle_frames(env.get_state(), rows, env.raster == 'alt')
    for k in FRAMES:
        same(tag + ': ' + k, rows, obs[k][_dev(env, rows)].cpu().numpy(), want[k])
    left = torch.stack([(obs[k] == SENT).any() for k in FRAMES])
    meter.tick()
    assert not left.any().item(), '%s: sentinel bytes left in %s' % (tag, [k for k, v in zip(FRAMES, left.tolist()) if v])


def _fill_sentinel(env):
    for k in FRAMES:
        env._observation()[k].fill_(SENT)


# ------------------------------------------------------------------------------------------------------------------------------ (a) large frames
@pytest.mark.parametrize('obs_mode,raster,N', [('pixels', 'ray', 1377), ('pixels_dirty', 'ray', 1377), ('pixels', 'alt', 2437)])
def test_large_frames_of_which_fewer_than_4096_fill_4_gib(obs_mode, raster, N):
    """255 x 255: 1 377 Ray frames are 4 297 892 400 bytes, 2 437 AltObs frames 4 295 358 720 -- the first batch sizes past 2^32 bytes, which went as ONE chunk of
    the sweep while its chunks were never fewer than 4 096 envs (its 32-bit byte count wrapped to less than one frame: reset() left the rest of the three
    arrays as they were).  Sentinel-filled arrays, reset(), then three steps with max_steps=3, which reset every env through the step path."""
    S, FB = 255, _frame_bytes(255, raster)
    assert N * FB >= 2 ** 32 > (N - 1) * FB
    meter = _Meter('large frames %s %s' % (obs_mode, raster), 5.5 * N * FB + 2 * GB)
    env, _, _ = make_env(N, obs_mode=obs_mode, raster=raster, seed=5, size=(S, S), max_steps=3)
    chunks, per = _chunks(env, FB)
    assert chunks == 2 and per < N
    rows = _rows_at(N, FB, chunks, per)
    assert {0, per - 1, per, N - 1, 2 ** 31 // FB, 2 ** 32 // FB} <= set(rows.tolist())
    _fill_sentinel(env)
    env.reset()
    _check_frame_arrays(env, rows, meter, 'reset', True)
    acts = torch.randint(0, 6, (3, N), device=env.device, dtype=torch.uint8, generator=torch.Generator(device='cuda').manual_seed(3))
    for t in range(3):
        env.step(acts[t])
    assert int(env.counters[1].item()) >= N                 # every env finished (timed out at the latest) and was reset by the step
    _check_frame_arrays(env, rows, meter, 'three steps', False)
    env.close()
    del env
    meter.done()


# ------------------------------------------------------------------------------------------------------------------------------ (b) many small frames
@pytest.mark.parametrize('rounds', [None, '0'])
def test_many_small_frames_in_two_chunks_with_a_ragged_second(rounds, monkeypatch):
    """90 001 frames of 32 x 32 (49 152 bytes): 4.42 GB, two chunks of 45 056 and 44 945 envs -- for the rounds' sake at the default
    CW_TUNE_RENDER_CHUNK_ROUNDS, by the rule's halving loop with 0 (no limit on the rounds: 90 112 envs pass 2^32 bytes).  The three assertions after reset()
    and after max_steps + 1 steps, and every reward, done and the end state of 512 envs on both sides of the chunk boundary and at both ends against the oracle."""
    N, S, T = 90001, 32, 4
    FB = _frame_bytes(S, 'ray')
    if rounds is not None:
        monkeypatch.setenv('CW_TUNE_RENDER_CHUNK_ROUNDS', rounds)
    meter = _Meter('small frames, rounds %s' % rounds, 5.5 * N * FB + 2 * GB)
    kw = dict(size=(S, S), max_steps=3)
    env, keys, pos = make_env(N, obs_mode='pixels', seed=7, **kw)
    chunks, per = _chunks(env, FB, 896 if rounds is None else int(rounds))
    assert (chunks, per) == (2, 45056)
    rows = _rows_at(N, FB, chunks, per)
    _fill_sentinel(env)
    env.reset()
    _check_frame_arrays(env, rows, meter, 'reset', True)
    acts = torch.randint(0, 6, (T, N), device=env.device, dtype=torch.uint8, generator=torch.Generator(device='cuda').manual_seed(4))
    r_host, d_host = record_steps(env, acts)
    _check_frame_arrays(env, rows, meter, 'four steps', False)
    idx = np.r_[0:128, per - 128:per + 128, N - 128:N]
    res = replay_against_oracle(env, keys, pos, oracle_kw(kw), acts.cpu().numpy(), r_host, d_host, frames=True, idx=idx)
    assert len(idx) == 512 and res['finished'] >= 512
    env.close()
    del env
    meter.done()


# ------------------------------------------------------------------------------------------------------------------------------ (c) per-env painters
def _changed_rows(a, b):
    """the rows in which two arrays of the same shape differ, found on the device"""
    return torch.nonzero((a != b).view(a.shape[0], -1).any(dim=1)).flatten().cpu().numpy()


def test_per_env_painters_at_an_env_offset_past_two_to_the_32():
    """The painters that take ONE env's frames (size_t offsets): reset_envs, imagine_obs(out=), snapshot_load and the terminal frame, in the dirty-cell engine of
    (a) with keep_terminal_obs, on the last env -- the one that holds byte 2^32 of every array -- and the one that holds byte 2^31.  The selected frames
    against the oracle / the model of imagine_obs; every other row of the engine's arrays and of the caller's is found unchanged on the device."""
    from oracle import OracleBatch
    N, S = 1377, 255
    FB = _frame_bytes(S, 'ray')
    sel = np.array(sorted({N - 1, 2 ** 32 // FB, 2 ** 31 // FB}))
    assert sel.tolist() == [688, 1376] and (N - 1) * FB < 2 ** 32 < N * FB
    meter = _Meter('per-env painters', 10.5 * N * FB + 2 * GB)
    kw = dict(size=(S, S), max_steps=5)
    env, keys, pos = make_env(N, obs_mode='pixels_dirty', seed=11, keep_terminal_obs=True, **kw)
    ora = OracleBatch(len(sel), rng_states=[(keys[i], int(pos[i])) for i in sel], **kw)
    env.reset()
    ora.reset()
    acts = torch.randint(0, 6, (9, N), device=env.device, dtype=torch.uint8, generator=torch.Generator(device='cuda').manual_seed(6))
    a_host = acts.cpu().numpy()
    for t in range(2):
        env.step(acts[t])
        ora.step(a_host[t, sel])
    same_states(env, ora, idx=sel, frames=tuple(FRAMES))
    obs = env._observation()
    # ---- reset_envs
    before = {k: obs[k].clone() for k in FRAMES}
    meter.tick()
    env.reset_envs(indices=sel.tolist())
    for e in ora.envs:
        e.reset()
    same_states(env, ora, idx=sel, frames=tuple(FRAMES), tag='reset_envs: ')
    for k in FRAMES:
        assert set(_changed_rows(obs[k], before[k]).tolist()) <= set(sel.tolist()), 'reset_envs wrote %s of an unselected env' % k
    assert set(_changed_rows(obs['observation'], before['observation']).tolist()) == set(sel.tolist())
    # ---- imagine_obs into a caller's array
    before = {k: obs[k].clone() for k in FRAMES}
    st0, (k0, p0) = env.get_state(), env.get_rng_states()
    out = torch.full((N,) + tuple(env.frame_shape), SENT, dtype=torch.uint8, device=env.device)
    meter.tick()
    got = env.imagine_obs(indices=sel.tolist(), out=out)
    assert got is out
    g, a, k2, p2 = model_imagine(st0, k0, p0, sel, st0['desired'])
    same('imagine_obs frames', sel, out[_dev(env, sel)].cpu().numpy(), np.stack([M.render(g[j], a[j]) for j in range(len(sel))]))
    written = torch.nonzero((out != SENT).view(N, -1).any(dim=1)).flatten().cpu().numpy()
    assert written.tolist() == sel.tolist(), 'imagine_obs wrote rows %s of the caller\'s array' % written.tolist()
    for k in FRAMES:
        assert torch.equal(obs[k], before[k]), 'imagine_obs without commit changed ' + k
    k1, p1 = env.get_rng_states()
    same('stream key after imagine_obs', sel, k1[sel], k2)
    same('stream position after imagine_obs', sel, p1[sel], p2)
    for j, e in enumerate(ora.envs):                         # (the oracle has no imagine_obs of a running episode: its streams follow the model's)
        e.set_rng(k2[j], int(p2[j]))
    del before, out, got
    # ---- the terminal frame of the step that ends the selected envs' episodes (five steps after their reset)
    ended = set()
    for t in range(2, 7):
        env.step(acts[t])
        _, o_done, _, term = ora.step(a_host[t, sel], details=True)
        same_terminal(env.terminal_observation, term, idx=sel, tag='step %d: ' % t)
        ended |= {int(sel[j]) for j in term}
    assert ended == set(sel.tolist())
    same_states(env, ora, idx=sel, frames=tuple(FRAMES), tag='after the terminal step: ')
    # ---- snapshot_save, two steps, snapshot_load: the frames at save time
    env.snapshot_reserve(len(sel))
    env.snapshot_save(envs=sel.tolist(), rows=list(range(len(sel))))
    saved = {k: obs[k][_dev(env, sel)].clone() for k in FRAMES}
    saved_state = {k: v[sel] for k, v in env.get_state().items()}
    for t in range(7, 9):
        env.step(acts[t])
    assert (env.get_state()['step_num'][sel] != saved_state['step_num']).all()
    before ={k: obs[k].clone() for k in FRAMES}
    meter.tick()
    env.snapshot_load(envs=sel.tolist(), rows=list(range(len(sel))))
    for k in FRAMES:
        assert torch.equal(obs[k][_dev(env, sel)], saved[k]), 'snapshot_load: ' + k
        assert set(_changed_rows(obs[k], before[k]).tolist()) <= set(sel.tolist()), 'snapshot_load wrote %s of an unselected env' % k
    want = _oracle_frames(saved_state, range(len(sel)), False)
    for k in FRAMES:
        same('snapshot_load: ' + k, sel, saved[k].cpu().numpy(), want[k])
    assert all(np.array_equal(v[sel], saved_state[k]) for k, v in env.get_state().items())
    del before, saved
    env.close()
    del env, obs
    meter.done()


# ------------------------------------------------------------------------------------------------------------------------------ (d) exports
def _one_hot_on_device(env):
    """obs_one_hot (ray.py:94-98) of every env, built with torch from grid() and get_state(): oracle_replay.one_hot_of on the device"""
    st = env.get_state()
    grid = env.grid()
    assert np.array_equal(grid.cpu().numpy(), st['grid'])
    N = env.num_envs
    oh = torch.zeros((N, env.size, env.size, 12), dtype=torch.uint8, device=env.device)
    for k in range(8):
        oh[..., k] = grid == k + 1
    r = torch.arange(N, device=env.device)
    a, h = _dev(env, st['agent_rc']), _dev(env, st['hold'])
    oh[r, a[:, 0], a[:, 1], 8] = 1
    oh[r[h > 0], a[h > 0, 0], a[h > 0, 1], 8 + h[h > 0]] = 1
    return oh, st


def test_one_hot_exports_past_two_to_the_32():
    """one_hot() of 5 505 envs of 255 x 255 is 4 295 551 500 bytes (cw_export_onehot), one_hot_states() of the same records as many (cw_export_onehot_states):
    both equal the one-hot built with torch from grid() and get_state()."""
    N, S = 5505, 255
    assert N * S * S * 12 == 4295551500 >= 2 ** 32 > (N - 1) * S * S * 12
    meter = _Meter('one-hot exports', 3.5 * N * S * S * 12 + 2 * GB)
    env, _, _ = make_env(N, obs_mode='state', seed=13, auto_reset=False, size=(S, S), max_steps=50)
    env.reset()
    acts = torch.randint(0, 6, (6, N), device=env.device, dtype=torch.uint8, generator=torch.Generator(device='cuda').manual_seed(8))
    for t in range(6):
        env.step(acts[t])
    want, st = _one_hot_on_device(env)
    rows = _rows_at(N, S * S * 12)
    same('the one-hot built with torch', rows, want[_dev(env, rows)].cpu().numpy(), one_hot_of(st['grid'][rows], st['agent_rc'][rows], st['hold'][rows]))
    got = env.one_hot()
    meter.tick()
    assert torch.equal(got, want), 'one_hot()'
    got.fill_(SENT)
    assert env.one_hot_states(env.hdr, env.slot_pos, out=got) is got
    meter.tick()
    assert torch.equal(got, want), 'one_hot_states()'
    for which, grid, agent in (('init', 'init_grid', 'init_agent_rc'), ('goal', 'goal_grid', 'goal_agent_rc')):        # the other two states of an env, its last rows
        oh = env.one_hot(out=got, which=which)
        same("one_hot(which='%s')" % which, rows, oh[_dev(env, rows)].cpu().numpy(), np.stack([M.one_hot(st[grid][i], st[agent][i]) for i in rows]))
    del got, want, oh
    env.close()
    del env
    meter.done()


@pytest.mark.parametrize('raster,N', [('ray', 689), ('alt', 689), ('alt', 1219)])
def test_int_image_of_one_hot_states_past_two_to_the_32(raster, N):
    """render_states(one_hot) writes int16 frames (cw_render_onehot): 689 of 255 x 255 in the Ray raster are 689 x 65 025 x 96 = 4 301 013 600 bytes, of AltObs
    1 219 (4 297 121 280; 689 are 2.4 GB).  No object is duplicated and what is held shows at the agent, so the image is render()'s, compared whole on the
    device in the Ray raster and in the rows at the ends of the array and around byte 2^31 and 2^32 with the oracle's rasteriser in both."""
    S, alt = 255, raster == 'alt'
    unit = 2 * _frame_bytes(S, raster)
    assert (N * unit >= 2 ** 32 > (N - 1) * unit) if (raster, N) != ('alt', 689) else N * unit > 2 ** 31
    meter = _Meter('int image %s %d' % (raster, N), 2.5 * N * unit + N * S * S * 12 + 2 * GB)
    env, _, _ = make_env(N, obs_mode='state', seed=17, auto_reset=False, raster=raster, size=(S, S), max_steps=50)
    env.reset()
    acts = torch.randint(0, 6, (6, N), device=env.device, dtype=torch.uint8, generator=torch.Generator(device='cuda').manual_seed(9))
    for t in range(6):
        env.step(acts[t])
    img = env.render_states(env.one_hot())
    meter.tick()
    assert img.dtype == torch.int16 and tuple(img.shape) == (N,) + tuple(env.frame_shape) and img.numel() * 2 == N * unit
    st = env.get_state()
    on = st['grid'][np.arange(N), st['agent_rc'][:, 0], st['agent_rc'][:, 1]]
    assert not ((st['hold'] == 1) & (on == 1)).any()         # (sticks held over sticks: the one pixel whose int value leaves a byte, AltObs)
    rows = _rows_at(N, unit)
    want = np.stack([_paint(st['grid'][i], st['agent_rc'][i], st['hold'][i], alt) for i in rows])
    same('render_states', rows, img[_dev(env, rows)].cpu().numpy(), want.astype(np.int16))
    shown = env.render()
    same('render()', rows, shown[_dev(env, rows)].cpu().numpy(), want)
    lo = 0                                                   # (the whole image against render(), a slice at a time: no second int16 array)
    while lo < N:
        assert torch.equal(img[lo:lo + 64], shown[lo:lo + 64].to(torch.int16)), 'render_states != render() in envs %d ..' % lo
        lo += 64
    meter.tick()
    del img, shown
    env.close()
    del env
    meter.done()
