"""GPU tier of cw_load_records_kernel through CraftingWorldVecEnv.load_records: packed records put back INTO envs, which then go on stepping.  Every load is
checked env by env with load_records_check.check_load_records (itself tested on the CPU, tests/test_load_records_logic.py) -- loaded envs against their
record, every other env and every other buffer byte for byte, the status bytes and counters[6] -- and the batch is then continued against the CPU oracle,
which is brought to the same states on the host by OracleEnv.update from the DECODED record (records_check.decode) and reads nothing of the engine but the
actions.  Every expectation comes from the oracle or from take() snapshots, never from the call under test.  Everything is bit-exact.  No timing."""
import numpy as np
import pytest
import torch

import engine_model as EM
import sequence_script as SS
from engines import ENGINES, K5, MENUS, N1, SIZES, k_of, n_cu
from load_records_check import BAD_INDEX, LOADED, MUTATIONS, NO_PART, REFUSED, check_load_records, mutated, walk_records
from load_records_model import model_for, pairs_script
from masked_check import masked_launch, spread, take
from oracle_replay import FRAMES, make_env, np_states, oracle_kw, same, same_states
from records_check import decode, encode
from recording_engine import RecordingLib
from state_tables import oracle_frame, painted_batch
from test_call_sequences import _compare, _drive
from test_masked_shapes import ALL_WIDTHS, _engine, _width
from test_snapshot import _step_recorded

pytestmark = pytest.mark.gpu

LOAD_ENGINES = dict(ENGINES, pixels_ray_auto=dict(obs_mode='pixels', raster='ray'))
T_ON = 2 * K5['max_steps'] + 3


def _dev(a, dtype=np.int32):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device='cuda')


def _pair(engine, base, S=5):
    """-> (env, its OracleBatch, pixels, alt), both reset"""
    from oracle import OracleBatch
    ekw, KW = dict(LOAD_ENGINES[engine]), k_of(S)
    raster, K = ekw.get('raster', 'ray'), ekw.get('fixed_init_state', 0)
    env, keys, pos = make_env(N1, *np_states(N1, base), **ekw, **KW)
    per_env = [MENUS[int(m)] for m in ekw['env_menu']] if 'env_menu' in ekw else [dict()] * N1
    ora = OracleBatch(N1, rng_states=list(zip(keys, pos)), per_env_kwargs=per_env, **oracle_kw(dict(KW, fixed_init_state=K), raster))
    env.reset()
    ora.reset()
    return env, ora, ekw['obs_mode'] != 'state', raster == 'alt'


def _walk(env, ora, T, seed):
    ora.rollout(spread(env, T, seed).astype(np.int8), nthreads=16)


def _oracle_takes(ora, hdr, slot_pos, src, status, S):
    """every env that loaded, brought to its record on the oracle's side: the DECODED record through OracleEnv.update"""
    good = np.flatnonzero(status == LOADED)
    d = decode(hdr[src[good]], slot_pos[src[good]], S)
    for j, i in enumerate(good.tolist()):
        ora.envs[i].update(grid=d['grid'][j], agent=d['agent'][j], hold=int(d['hold'][j]), achieved=int(d['achieved'][j]), desired=int(d['desired'][j]),
                           step_num=int(d['step_num'][j]))


def _load_checked(env, ora, hdr_t, pos_t, src, alt, S=5):
    """load_records(src) of device records, checked against the contract, then mirrored on the oracle -> the status bytes"""
    before = take(env)
    obs, status = env.load_records(hdr_t, pos_t, None if src is None else _dev(src), status=True)
    assert set(obs) == set(env._observation())
    after = take(env)
    h, p = hdr_t.cpu().numpy().reshape(-1, 16), pos_t.cpu().numpy().reshape(-1, 8).view(np.uint16)
    st = check_load_records(before, after, h, p, src, alt=alt, status=status.cpu().numpy())
    _oracle_takes(ora, h, p, np.arange(len(st)) if src is None else np.asarray(src), st, S)
    return st


def _continue(env, ora, pixels, seed, tag):
    acts = torch.randint(0, 6, (T_ON, N1), device='cuda', dtype=torch.uint8, generator=torch.Generator(device='cuda').manual_seed(seed))
    r_host, d_host = _step_recorded(env, acts)
    _, o_rew, o_done = ora.rollout(acts.cpu().numpy().astype(np.int8), nthreads=16, record=True)
    same('reward of every step after ' + tag, 0, r_host.T, o_rew.T)
    same('done of every step after ' + tag, 0, d_host.T, o_done.astype(bool).T)
    assert d_host.sum(axis=0).min() >= 2                          # every env has been reset twice since
    same_states(env, ora, frames=tuple(FRAMES) if pixels else (), tag='%d steps after %s: ' % (T_ON, tag))


# ------------------------------------------------------------------------------------------------------------------------------ 1. return to an earlier state
@pytest.mark.parametrize('engine', list(LOAD_ENGINES))
def test_return_to_an_earlier_state_then_continued_against_the_oracle(engine):
    env, ora, pixels, alt = _pair(engine, 33000)
    _walk(env, ora, 9, 1)
    rec_h, rec_p = env.hdr.clone(), env.slot_pos.clone()
    saved = take(env)
    ep_saved = np.array([e.view().ep_no for e in ora.envs])
    _walk(env, ora, 6, 2)                                         # (9 + 6 < max_steps: only a success ends an episode on the way)
    still = np.array([e.view().ep_no for e in ora.envs]) == ep_saved
    assert 40 <= still.sum()                                      # by the oracle alone
    src = np.where(still, np.arange(N1), -1).astype(np.int32)
    assert not np.array_equal(env.hdr.cpu().numpy()[still], saved['hdr'][still])
    st = _load_checked(env, ora, rec_h, rec_p, src, alt)
    assert np.array_equal(st == LOADED, still) and (st[~still] == NO_PART).all()
    after = take(env)
    for k in saved:                                               # the same episode: the env is where it was, whole
        if k.startswith('state_') or k in FRAMES or k in ('hdr', 'slot_pos'):     # (the mask OUTPUTS held a finished step's values where an env had just been reset)
            same('back where it was: ' + k, np.flatnonzero(still), after[k][still], saved[k][still])
    same_states(env, ora, frames=tuple(FRAMES) if pixels else (), tag='right after the load: ')
    _continue(env, ora, pixels, 3, 'the return')
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 2. commit a successor
@pytest.mark.parametrize('engine', list(LOAD_ENGINES))
def test_commit_a_successor_of_expand(engine):
    env, ora, pixels, alt = _pair(engine, 34000)
    _walk(env, ora, 5, 4)
    phase = (np.arange(N1) % K5['max_steps']).astype(np.int32)    # step_num 16 among them: their successors time out
    env.set_state(step_num=phase)
    for e, p in zip(ora.envs, phase):
        e.update(step_num=int(p))
    r = env.expand()
    acts = np.random.RandomState(5).randint(0, 6, N1)
    src = (acts * N1 + np.arange(N1)).astype(np.int32)            # row (a, j) into env j
    o_rew, o_done = ora.step(acts, auto_reset=False)              # the oracle stepped without auto-reset
    assert o_done.sum() >= 4
    before = take(env)
    hdr_t, pos_t = r['hdr'].reshape(6 * N1, 16), r['slot_pos'].reshape(6 * N1, 8)
    obs, status = env.load_records(hdr_t, pos_t, _dev(src), status=True)
    st = check_load_records(before, take(env), hdr_t.cpu().numpy(), pos_t.cpu().numpy(), src, alt=alt, status=status.cpu().numpy())
    assert (st == LOADED).all()
    same('reward of the committed successor', 0, r['reward'].cpu().numpy()[acts, np.arange(N1)], o_rew)
    same('done of the committed successor', 0, r['done'].cpu().numpy()[acts, np.arange(N1)], o_done)
    same_states(env, ora, frames=tuple(FRAMES) if pixels else (), tag='the committed successor, terminal ones included: ')
    _continue(env, ora, pixels, 6, 'the commit')
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 3. fork and permute
@pytest.mark.parametrize('engine', list(LOAD_ENGINES))
def test_fork_then_one_record_into_ten_envs_then_a_permutation(engine):
    env, ora, pixels, alt = _pair(engine, 35000)
    env.snapshot_reserve(2)
    _walk(env, ora, 5, 7)
    env.snapshot_save(envs=[3], rows=[0])
    twin = ora.envs[3].clone()
    env.snapshot_load(envs=list(range(10)), rows=[0] * 10, with_stream=False)
    for i in range(10):
        ora.envs[i].copy_from(twin, False)
    _walk(env, ora, 4, 8)                                         # ten envs of one episode walk apart
    rec_h, rec_p = env.hdr[:10].clone(), env.slot_pos[:10].clone()
    assert len({bytes(x) for x in rec_h.cpu().numpy()}) >= 5
    _walk(env, ora, 2, 9)
    src = np.full(N1, -1, np.int32)
    src[:10] = 4                                                  # one record into all ten
    st = _load_checked(env, ora, rec_h, rec_p, src, alt)
    assert (st[:10] == LOADED).all() and (st[10:] == NO_PART).all()
    assert len({bytes(x) for x in env.slot_pos[:10].cpu().numpy()}) == 1
    same_states(env, ora, frames=tuple(FRAMES) if pixels else (), tag='one record in ten envs: ')
    src[:10] = (np.arange(10) + 1) % 10                           # a cyclic permutation of their records
    st = _load_checked(env, ora, rec_h, rec_p, src, alt)
    assert (st[:10] == LOADED).all()
    same_states(env, ora, frames=tuple(FRAMES) if pixels else (), tag='a cyclic permutation of the records: ')
    _continue(env, ora, pixels, 10, 'the permutation')
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 4. refusals on the device
@pytest.mark.parametrize('engine', ['dirty_ray_auto', 'pixels_alt_auto'])
def test_indices_out_of_range_and_refused_records_leave_their_envs_alone(engine):
    """one launch: envs 0-19 take good records, envs 20-24 name -1, -7, R, R + 5 and 2^31 - 1, envs 30-45 one mutation of a good record each"""
    env, ora, pixels, alt = _pair(engine, 36000)
    _walk(env, ora, 6, 11)
    good_h, good_p = env.hdr[:30].clone(), env.slot_pos[:30].clone()
    muts = [mutated(name, 5) for name in MUTATIONS]
    hdr_t = torch.cat([good_h, _dev(np.stack([m[0] for m in muts]), np.uint8)]).contiguous()
    pos_t = torch.cat([good_p, _dev(np.stack([m[1] for m in muts]).view(np.int16), np.int16)]).contiguous()
    R = 30 + len(MUTATIONS)
    assert len(hdr_t) == R == 46
    _walk(env, ora, 5, 12)
    src = np.full(N1, -1, np.int64)
    src[:20] = (np.arange(20) * 7) % 30
    src[20:25] = (-1, -7, R, R + 5, 2 ** 31 - 1)
    src[30:30 + len(MUTATIONS)] = 30 + np.arange(len(MUTATIONS))
    skipped = env.snapshot_skipped
    st = _load_checked(env, ora, hdr_t, pos_t, src.astype(np.int32), alt)     # (refused envs byte for byte as before, frames included: check_load_records)
    assert st[:20].tolist() == [LOADED] * 20 and st[20:25].tolist() == [NO_PART, NO_PART, BAD_INDEX, BAD_INDEX, BAD_INDEX]
    assert st[30:46].tolist() == [REFUSED] * 16 and (st[46:] == NO_PART).all()
    assert env.snapshot_skipped == skipped + 3 + 16
    same_states(env, ora, frames=tuple(FRAMES), tag='after the mixed launch: ')
    _continue(env, ora, pixels, 13, 'the mixed launch')
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 5. every pixel kind
def _painted_records(S):
    """-> (hdr, slot_pos, grid, agent, hold) of N1 records: state_tables.painted_batch where it exists (S >= 5), below it the records of an oracle walk"""
    if S >= 5:
        _, grid, _, agent, hold = painted_batch(S, N1)
        z = np.zeros(N1, np.int64)
        hdr, pos = encode(dict(grid=grid, agent=agent, hold=hold, achieved=z, desired=z + 9, step_num=z + 3, flags=z))
        return hdr, pos, grid, agent.astype(np.int64), hold.astype(np.int64)
    hdr, pos = walk_records(S)
    pick = np.concatenate([np.flatnonzero(hdr[:, 2] != 0)[:N1 // 2], np.flatnonzero(hdr[:, 2] == 0)[:N1 - N1 // 2]])
    assert len(pick) == N1
    d = decode(hdr[pick], pos[pick], S)
    return hdr[pick], pos[pick], d['grid'], d['agent'], d['hold']


@pytest.mark.parametrize('size', SIZES)
@pytest.mark.parametrize('engine', ['dirty_ray_auto', 'pixels_ray_auto', 'pixels_alt_auto'])
def test_a_load_paints_every_state_class(engine, size):
    """host arrays, validated on the host and packed: obs is the oracle's frame of the state the record was made from, the init and goal frames stay"""
    ekw, alt = dict(LOAD_ENGINES[engine]), LOAD_ENGINES[engine].get('raster') == 'alt'
    hdr, pos, grid, agent, hold = _painted_records(size)
    env, _, _ = make_env(N1, *np_states(N1, 37000), **ekw, **k_of(size))
    env.reset()
    spread(env, 3, 14)
    before = take(env)
    obs, status = env.load_records(hdr, pos, status=True)          # record i for env i
    after = take(env)
    st = check_load_records(before, after, hdr, pos, None, alt=alt, status=status.cpu().numpy())
    assert (st == LOADED).all()
    want = np.stack([oracle_frame(grid[j], agent[j], hold[j], alt) for j in range(N1)])
    same('observation painted by the load', 0, obs['observation'].cpu().numpy(), want)
    for k in ('init_observation', 'desired_goal'):
        same(k + ' across the load', 0, after[k], before[k])
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 6. the dealer's edges
def _edge(name, N, epb, chunks):
    m = np.zeros(N, bool)
    if name == 'first_env':
        m[0] = True
    elif name == 'last_env':
        m[N - 1] = True
    elif name == 'one_whole_chunk':                               # (in the second-round case a chunk of the second round)
        c = chunks - 3
        m[c * epb:(c + 1) * epb] = True
        assert m.sum() == epb
    else:
        m[N // epb * epb:] = True
        assert name == 'last_partial_chunk' and 0 < m.sum() < epb
    return m


@pytest.mark.parametrize('width', ALL_WIDTHS)
def test_load_at_every_dealing_width(monkeypatch, width):
    """state mode, the batch sizes of tests/test_masked_shapes.py: src selects the first env, the last env, one whole chunk and the last partial chunk, each
    selected env taking the record of the env mirrored at the batch's middle"""
    N, epb, chunks = _width(width)
    env, _, _ = _engine(monkeypatch, N, obs_mode='state', auto_reset=False, **K5)
    assert masked_launch(N, n_cu(), 1)[:2] == (epb, chunks)
    env.reset()
    spread(env, 4, 15)
    rec_h, rec_p = env.hdr.clone(), env.slot_pos.clone()
    h, p = rec_h.cpu().numpy(), rec_p.cpu().numpy().view(np.uint16)
    spread(env, 3, 16)
    before = take(env)
    for name in ('first_env', 'last_env', 'one_whole_chunk', 'last_partial_chunk'):
        sel = np.flatnonzero(_edge(name, N, epb, chunks))
        src = np.full(N, -1, np.int32)
        src[sel] = N - 1 - sel
        _, status = env.load_records(rec_h, rec_p, _dev(src), status=True)
        after = take(env)
        st = check_load_records(before, after, h, p, src, status=status.cpu().numpy())
        assert np.flatnonzero(st == LOADED).tolist() == sel.tolist(), name
        before = after
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 7. capture
def test_load_and_step_captured_in_one_graph_with_the_records_rewritten_in_place():
    """torch.cuda.graph around load_records + step on a dirty-cell engine without auto-reset: capturing runs nothing, and two replays -- records, src and actions rewritten
    in place between them -- equal the eager sequence on a twin"""
    envs = []
    for _ in range(2):
        env, _, _ = make_env(N1, *np_states(N1, 38000), obs_mode='pixels_dirty', auto_reset=False, **K5)
        env.reset()
        envs.append(env)
    eager, cap = envs
    rounds = []
    for k in range(2):                                            # two sets of records, from the twins' own walk
        acts = spread(eager, 4, 17 + k)
        for t in range(len(acts)):
            cap.step(_dev(acts[t], np.uint8))
            cap.reset_envs(cap.done)
        rounds.append((eager.hdr.clone(), eager.slot_pos.clone(), _dev(np.random.RandomState(k).permutation(N1) + 5 * k),
                       _dev(np.random.RandomState(9 + k).randint(0, 6, N1), np.uint8)))
    torch.cuda.synchronize()
    start, twin = take(cap), take(eager)
    for k in start:
        assert np.array_equal(start[k], twin[k]), k
    rec_h, rec_p, src, act = (torch.empty_like(t) for t in rounds[0])
    for r in rounds:
        for buf, t in zip((rec_h, rec_p, src, act), r):
            buf.copy_(t)
        eager.load_records(rec_h, rec_p, src)
        eager.step(act)
    torch.cuda.synchronize()
    want = take(eager)
    cap.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap.load_records(rec_h, rec_p, src)
        cap.step(act)
    torch.cuda.synchronize()
    now = take(cap)
    for k in start:
        assert np.array_equal(now[k], start[k]), 'capturing ran something: ' + k
    for r in rounds:
        for buf, t in zip((rec_h, rec_p, src, act), r):
            buf.copy_(t)
        graph.replay()
    torch.cuda.synchronize()
    got = take(cap)
    assert not np.array_equal(want['hdr'], start['hdr']) and want['counters'][6] == start['counters'][6] + 5      # (round 1 names five records past the last)
    for k in want:
        assert np.array_equal(got[k], want[k]), 'two replays against the eager sequence: ' + k
    for env in envs:
        env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 8. the resident path
def test_single_env_with_host_outputs_on_the_resident_path():
    """N = 1, host_outputs, dirty-cell frames: the resident stepper is parked by the load and starts again from the record; status and frame are valid on
    the host when the call returns"""
    from gym_craftingworld_amd import _lib as L
    env, _, _ = make_env(1, *np_states(1, 7100), obs_mode='pixels_dirty', auto_reset=False, host_outputs=True, size=(5, 5), max_steps=30)
    assert env.tuner_state()['resident'] == 1
    env.reset()

    def step(a):
        L.check(env._lib.cw_step_resident(env._h, int(a), 0), 'cw_step_resident', env._lib)
        st = env.get_state()                                      # (parks the stepper)
        return int(env.reward[0]), bool(env.done[0]), st, env._obs.numpy().copy()
    for a in (1, 2, 4):
        step(a)
    st0, frame0, rec_h, rec_p = env.get_state(), env._obs.numpy().copy(), env.hdr.clone(), env.slot_pos.clone()
    first = step(0)
    step(3)
    step(5)
    assert not np.array_equal(env.hdr.cpu().numpy(), rec_h.cpu().numpy())
    obs, status = env.load_records(rec_h, rec_p, status=True)
    assert not status.is_cuda and status.tolist() == [LOADED]
    assert np.array_equal(obs['observation'].numpy(), frame0) and np.array_equal(env.hdr.cpu().numpy(), rec_h.cpu().numpy())
    st1 = env.get_state()
    for k in st0:
        assert np.array_equal(st1[k], st0[k]), k
    again = step(0)
    assert again[:2] == first[:2] and np.array_equal(again[3], first[3])
    for k in first[2]:
        assert np.array_equal(again[2][k], first[2][k]), k
    bad_h, bad_p = mutated('position S*S', 5)
    frame1, hdr1 = env._obs.numpy().copy(), env.hdr.cpu().numpy().copy()
    with pytest.raises(ValueError, match='record 0 cannot be loaded'):
        env.load_records(bad_h[None], bad_p[None])               # a host array: refused on the host
    obs, status = env.load_records(_dev(bad_h[None], np.uint8), _dev(bad_p[None].view(np.int16), np.int16), status=True)
    assert status.tolist() == [REFUSED] and np.array_equal(obs['observation'].numpy(), frame1) and np.array_equal(env.hdr.cpu().numpy(), hdr1)
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 9. error codes and the hand-over
def test_error_codes():
    from gym_craftingworld_amd import _lib as L
    N = 8
    rec_h, rec_p = torch.zeros((N + 1, 16), dtype=torch.uint8, device='cuda'), torch.zeros((N + 1, 8), dtype=torch.int16, device='cuda')
    src, status = torch.zeros(N + 1, dtype=torch.int32, device='cuda'), torch.zeros(N + 16, dtype=torch.uint8, device='cuda')
    fresh, _, _ = make_env(N, seed=3, obs_mode='state', auto_reset=False, **K5)
    with pytest.raises(L.CraftingWorldError, match=r'\(-3\)'):    # before the first reset
        fresh.load_records(rec_h[:N], rec_p[:N])
    fresh.close()
    env, _, _ = make_env(N, seed=3, obs_mode='state', auto_reset=False, **K5)
    env.reset()
    spread(env, 3, 1)
    before = take(env)
    H, P, SRC, ST = rec_h.data_ptr(), rec_p.data_ptr(), src.data_ptr(), status.data_ptr()

    def rc(s=SRC, h=H, p=P, n=N, st=ST, e=env._h):
        return env._lib.cw_load_records(e, s, h, p, n, st, env._stream())
    assert rc(n=0) == L.CW_OK and rc(s=None, n=0) == L.CW_ERR_INVALID
    for bad in (dict(e=None), dict(h=None), dict(p=None), dict(n=-1), dict(n=2 ** 27 + 1), dict(s=None, n=N - 1), dict(s=None, n=N + 1), dict(h=H + 8),
                dict(p=P + 8), dict(s=SRC + 2), dict(h=env.hdr.data_ptr()), dict(p=env.slot_pos.data_ptr()), dict(h=env.slot_pos.data_ptr()),
                dict(h=env.hdr.data_ptr() + 16 * (N - 1), n=1), dict(st=H + 16 * N - 1), dict(st=P), dict(st=SRC + 4 * N - 1), dict(st=SRC - N + 1)):
        assert rc(**bad) == L.CW_ERR_INVALID, bad
    with pytest.raises(ValueError, match='overlap the engine'):   # the engine's own buffers as records (CW_ERR_INVALID is a ValueError)
        env.load_records(env.hdr, env.slot_pos)
    with pytest.raises(ValueError):
        env.load_records(rec_h, rec_p)                            # N + 1 records without src
    torch.cuda.synchronize()
    after = take(env)
    for k in before:
        assert np.array_equal(after[k], before[k]), 'a refused call wrote ' + k
    assert rc(st=None) == L.CW_OK and rc(s=None, st=SRC) == L.CW_OK          # (all-zero records: refused by the rule, env by env)
    torch.cuda.synchronize()
    assert env.snapshot_skipped == int(before['counters'][6]) + 2 * N
    env.close()


def test_device_tensors_go_over_in_place_and_lists_are_packed():
    env, _, _ = make_env(N1, *np_states(N1, 39000), obs_mode='state', auto_reset=False, **K5)
    env.reset()
    spread(env, 3, 2)
    rec_h, rec_p = env.hdr.clone(), env.slot_pos.clone()
    src = _dev(np.arange(N1)[::-1])
    env._lib = RecordingLib(env._lib)
    _, status = env.load_records(rec_h, rec_p, src, status=True)
    (name, args), = env._lib.calls
    assert name == 'cw_load_records' and args[:5] == (src.data_ptr(), rec_h.data_ptr(), rec_p.data_ptr(), N1, status.data_ptr())
    env._lib.clear()
    env.load_records(rec_h.reshape(7, 10, 16), rec_p.reshape(7, 10, 8))                     # no src: NULL, record i for env i
    (name, args), = env._lib.calls
    assert args[:5] == (None, rec_h.data_ptr(), rec_p.data_ptr(), N1, None)
    env._lib.clear()
    env.load_records(rec_h, rec_p, [1, 0], envs=[3, 5])           # device records in place, the pairing packed on the host
    (name, args), = env._lib.calls
    assert args[1:4] == (rec_h.data_ptr(), rec_p.data_ptr(), N1) and args[0] not in (None, src.data_ptr())
    torch.cuda.synchronize()
    want = env.hdr.cpu().numpy()
    assert np.array_equal(want[3, :3], rec_h.cpu().numpy()[1, :3]) and np.array_equal(want[5, 4:], rec_h.cpu().numpy()[0, 4:])
    with pytest.raises(IndexError):
        env.load_records(rec_h, rec_p, [N1, 0], envs=[3, 5])
    env._lib.clear()
    env.load_records(rec_h[:, :].t().contiguous().t(), rec_p)     # a tensor that is not contiguous is copied through the host, and validated there
    (name, args), = env._lib.calls
    assert args[1] != rec_h.data_ptr() and args[2] != rec_p.data_ptr() and args[3] == N1
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 10. ordered pairs
@pytest.mark.parametrize('kind', SS.KINDS)
def test_load_records_before_and_after_every_state_changing_call(kind, tmp_path):
    """load_records paired with every mutator of the existing circuit (tests/sequence_script.py), in both orders and with itself; the engine against the
    extended CPU model (tests/load_records_model.py) after EVERY op, as tests/test_call_sequences.py compares"""
    S = 5
    ops = pairs_script(5, N1, K5['max_steps'], S, pooled=kind == 'state_auto_pool_menus')
    keys, pos = np_states(N1, SS.BASE)
    model, ekw = model_for(kind, S, keys, pos)
    env, _, _ = make_env(N1, keys, pos, **ekw)
    try:
        pixels = env.obs_mode != 'state'
        frames = tuple(FRAMES) if pixels else ()
        env.snapshot_reserve(SS.CAP)
        model.snapshot_reserve(SS.CAP)
        pend_model, pend_env, archive, n_loaded = [], [], None, 0
        for i, (name, args) in enumerate(ops):
            try:
                if name == 'archive':
                    archive = model.records()
                elif name == 'load_records':
                    hdr, slot_pos = archive[0].copy(), archive[1].copy()
                    hdr[0], slot_pos[0] = args['bad']
                    want = model.load_records(hdr, slot_pos, args['src'])
                    _, status = env.load_records(_dev(hdr, np.uint8), _dev(slot_pos.view(np.int16), np.int16), _dev(args['src']), status=True)
                    same('status', 0, status.cpu().numpy(), want)
                    n_loaded += int((want == LOADED).sum())
                else:
                    want = EM.apply(model, name, args, pend_model)
                    _drive(env, name, args, pend_env, tmp_path, None, None, want, pixels)
                _compare(env, model, frames)
            except AssertionError as err:
                raise AssertionError('%s: after op %s: %s' % (kind, SS.describe(ops, i), err)) from None
        assert n_loaded >= 24 * 30
    finally:
        env.close()
