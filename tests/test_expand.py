"""GPU tier of the one-step look-ahead: cw_expand_kernel / cw_export_onehot_states_kernel through CraftingWorldVecEnv.expand / one_hot_states.  Every call is
checked row by row with expand_check.check_expand (itself tested on the CPU, tests/test_expand_logic.py): every written row against the CPU oracle's
set_state + step, every row that must not be written against a sentinel, and the engine before and after the call byte for byte.  Everything is
bit-exact.  No timing."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from engines import ENGINES, K5, N1, SIZES, k_of, n_cu
from expand_check import FIELDS, LAYOUT, check_expand, oracle_successors
from masked_check import spread, take
from oracle_replay import make_env, np_states, one_hot_of, same
from records_check import DENSE, POS_HELD, decode
from records_gpu import SENT, caller_records, env_of_cases, host as _host, sentinel_out, walked_engine
from state_tables import local_table as _table, oracle_frame as _oracle_frame, table_coverage, table_desired, wall_table

pytestmark = pytest.mark.gpu

_WIDTH = {'reward': 4, 'done': 1, 'changed': 1, 'achieved_mask': 2, 'hdr': 16, 'slot_pos': 16}
_DTYPE = {'reward': torch.int32, 'done': torch.bool, 'changed': torch.bool, 'achieved_mask': torch.int16, 'hdr': torch.uint8, 'slot_pos': torch.int16}


def _sentinel_out(M):
    """output buffers as expand(out=...) takes them, every byte SENT"""
    return sentinel_out(LAYOUT, _WIDTH, _DTYPE, M)


def _dense_of(snap):
    return decode(snap['hdr'], snap['slot_pos'], snap['state_grid'].shape[1])


# ------------------------------------------------------------------------------------------------------------------------------ 1. the whole local transition table
S1, MAX1 = 5, 9


@functools.lru_cache(maxsize=None)
def _table_desired():
    """desired of env i: for half of the envs (RandomState(1)) the achieved mask the oracle gets for action i % 6, else randint(1, 512)"""
    grid, init, agent, hold, ach = _table()
    n = len(hold)
    z = np.zeros(n, np.int64)
    suc = oracle_successors(dict(grid=grid, agent=agent, hold=hold, achieved=ach, desired=z + 1, step_num=z + 3, flags=z), init, dict(size=(S1, S1), max_steps=MAX1))
    rng = np.random.RandomState(1)
    return np.array([int(suc['achieved'][i % 6, i]) if rng.rand() < 0.5 else rng.randint(1, 512) for i in range(n)], np.int64)


@pytest.mark.parametrize('step_num', [3, MAX1 - 1])
@pytest.mark.parametrize('style', [None, 'subset'])
def test_the_whole_local_transition_table(style, step_num):
    """18 816 states, one env each, injected with set_state; all six successors of every one against the oracle, under both reward rules, mid-episode and
    one step before the time-out.  What the table exercises is counted from the oracle's values alone, before anything is compared."""
    from gym_craftingworld_amd import CraftingWorldVecEnv
    grid, init, agent, hold, ach = _table()
    des = _table_desired()
    n = len(hold)
    okw = dict(size=(S1, S1), max_steps=MAX1)
    env = CraftingWorldVecEnv(n, obs_mode='state', reward_style=style, auto_reset=False, seed=5, **okw)
    env.reset()
    env.set_state(grid=grid, init_grid=init, agent_rc=agent.astype(np.uint8), hold=hold.astype(np.uint8), achieved=ach.astype(np.uint16),
                  desired=des.astype(np.uint16), step_num=np.full(n, step_num, np.int32))
    before = take(env)
    flags = _dense_of(before)['flags']                                     # (of a record only its flag word is the engine's: the reward rule, no success yet)
    assert ((flags & ~1) == (2 if style else 0)).all()
    states = dict(grid=grid, agent=agent, hold=hold, achieved=ach, desired=des, step_num=np.full(n, step_num, np.int64), flags=flags)
    suc = oracle_successors(states, init, okw)
    gained, lost = suc['achieved'] & ~ach, ach & ~suc['achieved']
    gains = [int(((gained >> b) & 1).sum()) for b in range(9)]
    losses = [int(((lost >> b) & 1).sum()) for b in range(5, 9)]
    success = int((suc['reward'] == MAX1).sum())
    timeout_only = int((suc['done'] & (suc['reward'] != MAX1)).sum())
    print('gains', gains, 'losses of bits 5..8', losses, 'successes', success, 'changed', int(suc['changed'].sum()), 'unchanged', int((~suc['changed']).sum()),
          'done by time-out alone', timeout_only)
    assert min(gains) >= 100 and min(losses) >= 400 and success >= 10000
    assert suc['changed'].sum() >= 50000 and (~suc['changed']).sum() >= 50000
    if step_num == MAX1 - 1:
        assert timeout_only >= 80000
    r = env.expand()
    after = take(env)
    assert tuple(r['hdr'].shape) == (6, n, 16) and r['achieved_mask'].dtype == env.achieved_mask.dtype and r['done'].dtype == torch.bool
    part, skipped = check_expand(before, after, None, None, _host(r), SENT, oracle_kw=okw, successors=(states, suc))
    assert (part, skipped) == (n, 0)
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 1b. the table at every wall, and on large grids
WALL_S = 8
WALL_ANCHORS = [(0, 0), (0, 7), (7, 0), (7, 7), (0, 4), (4, 7), (7, 4), (4, 0)]     # the four corners and the four mid-edge cells


@functools.lru_cache(maxsize=None)
def _wall_table():
    table = wall_table(WALL_S, WALL_ANCHORS, 75264, span='full')
    return table, table_desired(table, dict(size=(WALL_S, WALL_S), max_steps=MAX1))


@pytest.mark.parametrize('style', [None, 'subset'])
def test_the_wall_table_on_every_wall(style):
    """The table of test_the_whole_local_transition_table with the agent in each corner and in the middle of each edge of an 8 x 8 grid: 8 x 9 408 = 75 264
    states, one env each.  Every move runs into its wall (the min(.., S - 1) clamp of Right and Down among them) and eval_task_edit follows the blocked
    move; Right and Down are expand's own instances of the step.  What the table exercises is counted from the oracle's values before anything is compared."""
    from gym_craftingworld_amd import CraftingWorldVecEnv
    (grid, init, agent, hold, ach), des = _wall_table()
    n = len(hold)
    assert n == 75264
    okw = dict(size=(WALL_S, WALL_S), max_steps=MAX1)
    env = CraftingWorldVecEnv(n, obs_mode='state', reward_style=style, auto_reset=False, seed=5, **okw)
    env.reset()
    env.set_state(grid=grid, init_grid=init, agent_rc=agent.astype(np.uint8), hold=hold.astype(np.uint8), achieved=ach.astype(np.uint16),
                  desired=des.astype(np.uint16), step_num=np.full(n, 3, np.int32))
    before = take(env)
    flags = _dense_of(before)['flags']
    assert ((flags & ~1) == (2 if style else 0)).all()
    states = dict(grid=grid, agent=agent, hold=hold, achieved=ach, desired=des, step_num=np.full(n, 3, np.int64), flags=flags)
    suc = oracle_successors(states, init, okw)
    cov = table_coverage(states, suc)
    success = int((suc['reward'] == MAX1).sum())
    print(cov, 'successes', success)
    assert min(cov['gains']) >= 100 and min(cov['losses']) >= 400 and cov['changed'] >= 50000 and cov['unchanged'] >= 50000
    assert min(cov['blocked_moves']) >= 10000 and success >= 10000
    r = env.expand()
    after = take(env)
    part, skipped = check_expand(before, after, None, None, _host(r), SENT, oracle_kw=okw, successors=(states, suc))
    assert (part, skipped) == (n, 0)
    env.close()


@pytest.mark.parametrize('S', [182, 255])
def test_the_far_corner_table_on_large_grids(S):
    """432 states at the three far corners of a 182 x 182 / 255 x 255 grid, one env each: slot cells above 32 767 (negative in the int16 tensors), rows and
    columns above 127, the held / gone marks 510 above the largest cell.  Depth 1 against the oracle; depth 2 -- expand() of its own records -- for the
    successors of Right and Down; the host path (slot_pos as numpy uint16) against the in-place one; one_hot_states of 864 records, several rounds of the
    export's grid-stride loop; render_states of four of them."""
    from gym_craftingworld_amd import CraftingWorldVecEnv
    grid, init, agent, hold, ach = wall_table(S, [(S - 1, S - 1), (0, S - 1), (S - 1, 0)], 512)
    n = len(hold)
    assert n == 432
    okw = dict(size=(S, S), max_steps=MAX1)
    des = np.where((np.arange(n) % 2 == 0) & (ach != 0), ach, np.random.RandomState(S).randint(1, 512, n))      # every other goal: keep what is achieved
    env = CraftingWorldVecEnv(n, obs_mode='state', auto_reset=False, seed=6, **okw)
    env.reset()
    env.set_state(grid=grid, init_grid=init, agent_rc=agent.astype(np.uint8), hold=hold.astype(np.uint8), achieved=ach.astype(np.uint16),
                  desired=des.astype(np.uint16), step_num=np.full(n, 3, np.int32))
    before = take(env)
    s0 = dict(grid=grid, agent=agent, hold=hold, achieved=ach, desired=des, step_num=np.full(n, 3, np.int64), flags=_dense_of(before)['flags'])
    suc1 = oracle_successors(s0, init, okw)
    cov = table_coverage(s0, suc1)
    above = int(((before['slot_pos'].view(np.uint16) > 32767) & (before['slot_pos'].view(np.uint16) < POS_HELD)).sum())
    print(S, cov, 'slot cells above 32 767:', above, 'successes', int((suc1['reward'] == MAX1).sum()))
    assert min(cov['gains']) >= 2 and min(cov['losses']) >= 10 and min(cov['blocked_moves']) >= 100 and cov['pickups'] >= 40 and cov['drops'] >= 40
    assert above >= 300 and (agent.max(axis=1) >= 128).all() and (before['slot_pos'] < -2).sum() == above and (suc1['reward'] == MAX1).sum() >= 20
    r1 = env.expand()
    assert r1['slot_pos'].dtype == torch.int16
    part, skipped = check_expand(before, take(env), None, None, _host(r1), SENT, oracle_kw=okw, successors=(s0, suc1))
    assert (part, skipped) == (n, 0)
    # ---- depth 2: 2 592 input states, the rows of the successors of Right and Down against the oracle
    r2 = env.expand(hdr=r1['hdr'], slot_pos=r1['slot_pos'])
    assert tuple(r2['hdr'].shape) == (6, 6 * n, 16)
    after = take(env)
    h1, h2 = _host(r1), _host(r2)
    for a in (1, 2):
        s1 = {k: suc1[k][a] for k in DENSE}
        suc2 = oracle_successors(s1, init, okw)
        part, _ = check_expand(before, after, dict(hdr=h1['hdr'][a], slot_pos=h1['slot_pos'][a]), None, {f: v[:, a * n:(a + 1) * n] for f, v in h2.items()}, SENT,
                               oracle_kw=okw, successors=(s1, suc2))
        assert part == n
    host = env.expand(hdr=r1['hdr'], slot_pos=h1['slot_pos'].view(np.uint16))          # the host path: validated, copied, the same bytes
    for f in FIELDS:
        assert torch.equal(host[f], r2[f]), f
    del r2, host, h2
    # ---- the one-hot view of the successors of Up and Right: more than one round of the export's grid-stride loop
    assert 2 * n * S * S > n_cu() * 32 * 256
    oh = env.one_hot_states(r1['hdr'][:2], r1['slot_pos'][:2])
    assert tuple(oh.shape) == (2, n, S, S, 12)
    for a in range(2):
        same('one_hot_states of the successors of action %d' % a, 0, oh[a].cpu().numpy(), one_hot_of(suc1['grid'][a], suc1['agent'][a], suc1['hold'][a]))
    frames = env.render_states(oh[0, :4])
    img = np.stack([_oracle_frame(suc1['grid'][0, j], suc1['agent'][0, j], suc1['hold'][0, j], False) for j in range(4)])
    same('render_states of the successors', 0, (frames.cpu().numpy() & 0xFF).astype(np.uint8), img)
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 2. against the engine's own step; 6. one-hot and frames
def _against_the_engines_own_step(engine, S):
    """expand() of the current states, then the same successors the long way round: snapshot_save once, and for each action snapshot_load(with_stream=True)
    + step.  Without auto-reset the step's hdr, slot_pos, reward, done and achieved_mask equal row a of the result byte for byte; with auto-reset the
    outputs do everywhere and the records where the env did not finish -- the finished ones are the terminal states only expand() shows, checked against
    the oracle.  The one-hot view and the frame of every successor equal the oracle's."""
    ekw, K = dict(ENGINES[engine]), k_of(S)
    alt = ekw.get('raster', 'ray') == 'alt'
    env, _, _ = make_env(N1, *np_states(N1, 52000), **ekw, **K)
    env.snapshot_reserve(N1)
    env.reset()
    spread(env, 9, 1)
    sn = env.get_state()['step_num']
    sn[::5] = K['max_steps'] - 1                                 # every fifth env one step before the time-out: successors that end the episode
    env.set_state(step_num=sn)
    before = take(env)
    states = _dense_of(before)
    suc = oracle_successors(states, before['state_init_grid'], K)
    assert suc['done'][:, ::5].all() and not suc['done'].all()
    r = env.expand()
    after = take(env)                                             # (every buffer, stream, frame and counter: check_expand compares them all)
    check_expand(before, after, None, None, _host(r), SENT, oracle_kw=K, successors=(states, suc))
    rows = torch.arange(N1, dtype=torch.int32, device='cuda')
    env.snapshot_save(rows)
    for a in range(6):
        env.snapshot_load(rows, with_stream=True)
        _, rew, done, _ = env.step(torch.full((N1,), a, dtype=torch.uint8, device='cuda'))
        assert torch.equal(rew.to(r['reward'].device), r['reward'][a]) and torch.equal(done.to(r['done'].device), r['done'][a]), a
        assert torch.equal(env.achieved_mask.to(r['achieved_mask'].device), r['achieved_mask'][a]), a
        same('done of action %d' % a, 0, done.cpu().numpy(), suc['done'][a])
        keep = torch.ones(N1, dtype=torch.bool, device='cuda') if not env.auto_reset else ~r['done'][a]
        assert keep.any()
        assert torch.equal(env.hdr[keep], r['hdr'][a][keep]) and torch.equal(env.slot_pos[keep], r['slot_pos'][a][keep]), a
        if env.auto_reset:                                        # the terminal states: the oracle's (check_expand has compared them; here by name)
            fin = np.flatnonzero(suc['done'][a])
            got = decode(r['hdr'][a].cpu().numpy()[fin], r['slot_pos'][a].cpu().numpy()[fin], S)
            for k in DENSE:
                same('terminal %s of action %d' % (k, a), fin, got[k], suc[k][a][fin])
    # ---- 6. the one-hot view and the frame of every successor
    oh = env.one_hot_states(r['hdr'], r['slot_pos'])
    assert tuple(oh.shape) == (6, N1, S, S, 12) and oh.dtype == torch.uint8
    want = one_hot_of(suc['grid'].reshape(6 * N1, S, S), suc['agent'].reshape(6 * N1, 2), suc['hold'].reshape(6 * N1))
    same('one_hot_states of the successors', 0, oh.cpu().numpy().reshape(6 * N1, S, S, 12), want)
    frames = env.render_states(oh.reshape(6 * N1, S, S, 12)[:64])
    img = np.stack([_oracle_frame(suc['grid'].reshape(-1, S, S)[j], suc['agent'].reshape(-1, 2)[j], suc['hold'].reshape(-1)[j], alt) for j in range(64)])
    same('render_states of the successors', 0, (frames.cpu().numpy() & 0xFF).astype(np.uint8), img)
    assert torch.equal(env.one_hot_states(env.hdr, env.slot_pos), env.one_hot())
    env.close()


@pytest.mark.parametrize('engine', list(ENGINES))
def test_against_the_engines_own_step_on_packed_bytes(engine):
    _against_the_engines_own_step(engine, 5)


@pytest.mark.parametrize('size', [x for x in SIZES if x != 5])
@pytest.mark.parametrize('engine', list(ENGINES))
def test_against_the_engines_own_step_on_packed_bytes_at_size(engine, size):
    """the same on 4 x 4, 7 x 7, 8 x 8 and 21 x 21 grids: below, at and above the size at which the full-frame engine changes painter, and the headline frame"""
    _against_the_engines_own_step(engine, size)


def test_host_outputs_engine():
    """an engine whose outputs live in mapped host memory: the same call, synchronised on return"""
    env, _, _ = make_env(4, *np_states(4, 53000), obs_mode='pixels_dirty', host_outputs=True, auto_reset=False, **K5)
    env.reset()
    for a in (1, 2, 4, 1, 5, 0):
        env.step(np.full(4, a, np.int32))
    before = take(env)
    r = env.expand()
    check_expand(before, take(env), None, None, _host(r), SENT, oracle_kw=K5)
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 3. shapes and edges
@pytest.fixture(scope='module')
def engine70():
    env = walked_engine(54000, 9)
    yield env
    env.close()


@pytest.mark.parametrize('M', [1, 63, 64, 65, 257, 1000])
def test_shapes_and_edges(engine70, M):
    """M states taken from a 70-env engine, env_of on the device and handed over in place: every written and every unwritten row, and the skipped states
    counted once each -- not once per action"""
    env = engine70
    e = env_of_cases(M, N1)
    src = np.where((e >= 0) & (e < N1), e, 0)
    before = take(env)
    hdr, pos = caller_records(before, e, M, N1, K5['max_steps'])
    t_hdr, t_pos, t_env = torch.as_tensor(hdr, device='cuda'), torch.as_tensor(pos, device='cuda'), torch.as_tensor(e.astype(np.int32), device='cuda')
    out = _sentinel_out(M)
    skipped0 = env.expand_skipped
    r = env.expand(t_hdr, t_pos, t_env, out=out)
    assert all(r[f] is out[f] for f in FIELDS)
    part, skipped = check_expand(before, take(env), dict(hdr=hdr, slot_pos=pos), e, _host(out), SENT, oracle_kw=K5)
    assert skipped == int((e >= N1).sum()) and part == int(((e >= 0) & (e < N1)).sum())
    assert env.expand_skipped == skipped0 + skipped
    with pytest.raises(IndexError) if skipped else pytest.raises(ValueError):     # the host-validated path refuses what the kernel skips
        env.expand(hdr, pos, e if skipped else e[:-1])
    if M == 65:                                                                   # every single field: the other buffers stay as they were
        for f in FIELDS:
            bufs = _sentinel_out(M)
            before = take(env)
            r = env.expand(t_hdr, t_pos, t_env, fields=[f], out={f: bufs[f]})
            assert list(r) == [f]
            check_expand(before, take(env), dict(hdr=hdr, slot_pos=pos), e, _host(r), SENT, oracle_kw=K5)
            for g in FIELDS:
                if g != f:
                    assert bool((bufs[g].view(torch.uint8) == SENT).all()), (f, g)
        r = env.expand(hdr, pos, np.where(e >= N1, -1, e))                        # numpy in: validated and copied by the host
        live = torch.as_tensor(src == e, device='cuda')
        assert all(torch.equal(r[f][:, live], out[f][:, live]) for f in FIELDS)


def test_no_states_and_bad_arguments_of_the_method(engine70):
    env = engine70
    r = env.expand(hdr=torch.empty((0, 16), dtype=torch.uint8, device='cuda'), slot_pos=torch.empty((0, 8), dtype=torch.int16, device='cuda'))
    assert set(r) == set(FIELDS) and all(t.shape[:2] == (6, 0) and t.device == env.device for t in r.values())
    assert tuple(env.one_hot_states(np.zeros((0, 16), np.uint8), np.zeros((0, 8), np.int16)).shape) == (0, 5, 5, 12)
    good = env.expand()
    for bad in (dict(fields=[]), dict(fields=['reward', 'frames']), dict(fields=['done', 'done']), dict(hdr=env.hdr), dict(slot_pos=env.slot_pos),
                dict(env_of=torch.zeros(N1, dtype=torch.int32, device='cuda')), dict(out={'reward': good['reward']}),
                dict(out=dict(good, reward=good['reward'].to(torch.int64))), dict(out=dict(good, hdr=good['hdr'][:, :, :8])),
                dict(out=dict(good, done=good['done'].cpu())), dict(hdr=env.hdr, slot_pos=env.slot_pos, out=dict(good, done=good['done'][:, :5])),
                dict(hdr=env.hdr[:5], slot_pos=env.slot_pos)):
        with pytest.raises(ValueError):
            env.expand(**bad)


# ------------------------------------------------------------------------------------------------------------------------------ 4. depth 2 with no index array
def test_depth_two_with_no_index_array():
    """expand() of expand()'s own records: 36 N rows, each against the oracle stepped twice from the env's state -- a done state just steps on"""
    env, _, _ = make_env(N1, *np_states(N1, 55000), obs_mode='state', auto_reset=False, **K5)
    env.reset()
    spread(env, K5['max_steps'] - 1, 4)                           # envs that have not succeeded on the way stand one step before the time-out
    before = take(env)
    s0 = _dense_of(before)
    suc1 = oracle_successors(s0, before['state_init_grid'], K5)
    assert suc1['done'].any()                                     # (the oracle alone: first steps that end the episode)
    s1 = {k: suc1[k].reshape((6 * N1,) + suc1[k].shape[2:]) for k in DENSE}
    suc2 = oracle_successors(s1, np.tile(before['state_init_grid'], (6, 1, 1)), K5)
    assert (suc2['step_num'].reshape(6, 6, N1) == s0['step_num'] + 2).all() and suc2['done'].reshape(6, 6, N1)[:, suc1['done']].any()
    r1 = env.expand()
    r2 = env.expand(**{k: r1[k] for k in ('hdr', 'slot_pos')})
    assert tuple(r2['hdr'].shape) == (6, 6 * N1, 16) and tuple(r2['reward'].shape) == (6, 6 * N1)
    inputs = dict(hdr=r1['hdr'].cpu().numpy().reshape(-1, 16), slot_pos=r1['slot_pos'].cpu().numpy().reshape(-1, 8))
    part, _ = check_expand(before, take(env), inputs, None, _host(r2), SENT, oracle_kw=K5, successors=(s1, suc2))
    assert part == 6 * N1
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 5. capture
def test_captured_into_a_graph():
    """torch.cuda.graph around one expand(out=...): the call only enqueues; replayed after the env has stepped it equals an eager expand() of the new state"""
    N = 300
    env, _, _ = make_env(N, *np_states(N, 56000), obs_mode='state', **K5)
    env.reset()
    spread(env, 5, 6)
    out = _sentinel_out(N)
    env.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.expand(out=out)
    assert all(bool((t.view(torch.uint8) == SENT).all()) for t in out.values())          # (capturing ran nothing)
    for rnd in range(3):
        spread(env, 3, 7 + rnd)
        g.replay()
        eager = env.expand()
        for f in FIELDS:
            assert torch.equal(out[f], eager[f]), (rnd, f)
    before = take(env)
    g.replay()
    torch.cuda.synchronize()
    check_expand(before, take(env), None, None, _host(out), SENT, oracle_kw=K5)
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 7. call order and arguments through ctypes
def test_call_order_and_arguments_through_ctypes():
    from gym_craftingworld_amd import CraftingWorldVecEnv, _lib as L
    N = 8
    env = CraftingWorldVecEnv(N, obs_mode='state', auto_reset=False, seed=3, **K5)
    lib, h, st = env._lib, env._h, env._stream()
    bufs = _sentinel_out(N)
    vp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    full = L.cw_expand_out(reward=vp(bufs['reward']), done=vp(bufs['done']), changed=vp(bufs['changed']), achieved=vp(bufs['achieved_mask']),
                           hdr=vp(bufs['hdr']), slot_pos=vp(bufs['slot_pos']))
    oh = torch.empty((N, 5, 5, 12), dtype=torch.uint8, device='cuda')
    assert lib.cw_expand(h, None, None, None, N, C.byref(full), st) == L.CW_ERR_STATE and b'before cw_reset' in lib.cw_last_error()
    assert lib.cw_export_onehot_states(h, vp(env.hdr), vp(env.slot_pos), N, vp(oh), st) == L.CW_ERR_STATE and b'before cw_reset' in lib.cw_last_error()
    env.reset()
    hdr, pos, eo = vp(env.hdr), vp(env.slot_pos), vp(torch.zeros(N, dtype=torch.int32, device='cuda'))
    assert lib.cw_expand(h, None, None, None, N, C.byref(full), st) == L.CW_OK
    assert lib.cw_expand(h, None, hdr, pos, 0, C.byref(full), st) == L.CW_OK                    # no states: nothing enqueued
    one = lambda **kw: L.cw_expand_out(**kw)  # noqa: E731
    invalid = [((None, None, None, None, N, C.byref(full)), b'engine'),
               ((h, None, None, None, N, None), b'out'),
               ((h, None, None, None, N, C.byref(one())), b'every field'),
               ((h, None, hdr, pos, -1, C.byref(full)), b'n_states'),
               ((h, None, hdr, pos, 2 ** 27 + 1, C.byref(full)), b'n_states'),
               ((h, None, None, None, N - 1, C.byref(full)), b'num_envs'),
               ((h, None, None, None, 6 * N, C.byref(full)), b'num_envs'),
               ((h, None, hdr, None, N, C.byref(full)), b'hdr_in given without slot_pos_in'),
               ((h, None, None, pos, N, C.byref(full)), b'slot_pos_in given without hdr_in'),
               ((h, eo, None, None, N, C.byref(full)), b'env_of'),
               ((h, None, vp(env.hdr, 8), pos, N - 1, C.byref(full)), b'hdr_in is not 16-byte aligned'),
               ((h, None, hdr, vp(env.slot_pos, 2), N - 1, C.byref(full)), b'slot_pos_in is not 16-byte aligned'),
               ((h, None, hdr, pos, N - 1, C.byref(one(hdr=vp(bufs['hdr'], 4)))), b'out->hdr is not 16-byte aligned'),
               ((h, None, hdr, pos, N - 1, C.byref(one(reward=vp(bufs['reward']), slot_pos=vp(bufs['slot_pos'], 8)))), b'out->slot_pos is not 16-byte aligned')]
    for args, word in invalid:
        assert lib.cw_expand(*args, st) == L.CW_ERR_INVALID, word
        assert word in lib.cw_last_error(), (word, lib.cw_last_error())
    for args, word in [((None, hdr, pos, N, vp(oh)), b'engine'), ((h, None, pos, N, vp(oh)), b'hdr'), ((h, hdr, None, N, vp(oh)), b'slot_pos'),
                       ((h, hdr, pos, N, None), b'out'), ((h, hdr, pos, -1, vp(oh)), b'n_states'), ((h, hdr, pos, 2 ** 27 + 1, vp(oh)), b'n_states'),
                       ((h, vp(env.hdr, 1), pos, N - 1, vp(oh)), b'hdr is not 16-byte aligned'),
                       ((h, hdr, vp(env.slot_pos, 6), N - 1, vp(oh)), b'slot_pos is not 16-byte aligned')]:
        assert lib.cw_export_onehot_states(*args, st) == L.CW_ERR_INVALID, word
        assert word in lib.cw_last_error(), (word, lib.cw_last_error())
    assert lib.cw_export_onehot_states(h, hdr, pos, 0, vp(oh), st) == L.CW_OK
    torch.cuda.synchronize()
    assert env.expand_skipped == 0
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 8. the view kernels past their first round
def test_grid_and_one_hot_exports_past_their_first_round():
    """cw_export_grid_kernel / cw_export_onehot_kernel launch at most n_cu * 32 workgroups of 256 threads, one cell each, and loop: on a 255 x 255 grid with
    3 envs more than one round holds, the second trip of the loop writes the last envs.  grid() and one_hot() of the current, goal and init state
    against get_state()."""
    S = 255
    per_round = n_cu() * 32 * 256
    N = -(-per_round // (S * S)) + 3
    assert N * S * S > per_round and (N - 3) * S * S >= per_round                  # (the last three envs lie wholly in the second round)
    env, _, _ = make_env(N, *np_states(N, 57000), obs_mode='state', size=(S, S), max_steps=17)
    env.reset()
    spread(env, 3, 9)
    st = env.get_state()
    assert (st['agent_rc'] != st['init_agent_rc']).any() and len({tuple(a) for a in st['agent_rc'].tolist()}) > N // 2
    same('grid()', 0, env.grid().cpu().numpy(), st['grid'])
    for which, g, a, h in (('current', 'grid', 'agent_rc', st['hold']), ('goal', 'goal_grid', 'goal_agent_rc', np.zeros(N, np.uint8)),
                           ('init', 'init_grid', 'init_agent_rc', np.zeros(N, np.uint8))):
        same('one_hot(which=%r)' % which, 0, env.one_hot(which=which).cpu().numpy(), one_hot_of(st[g], st[a], h))
    env.close()


@pytest.mark.parametrize('raster', ['ray', 'alt'])
def test_render_states_past_its_first_round(raster):
    """cw_render_onehot_kernel / cw_render_onehot_alt_kernel launch at most 1 024 workgroups -- 4 096 waves, one state each -- and loop: 4 099 states of
    4 x 4 cells, random contents as test_hip_parity.test_render_of_arbitrary_one_hot_states draws them, against the numpy restatements of the reference's
    render(state); the last three, the second round, by name."""
    from test_hip_parity import _reference_alt_render_of_any_state, _reference_render_of_any_state
    ref = _reference_alt_render_of_any_state if raster == 'alt' else _reference_render_of_any_state
    S, M = 4, 4099
    assert M > 1024 * 4
    rng = np.random.RandomState(13)
    states = (rng.rand(M, S, S, 12) < np.array([0.02, 0.3, 0.08])[np.arange(M) % 3][:, None, None, None]).astype(np.uint8)
    states[..., 8] = 0
    for _ in range(3):
        on = np.flatnonzero(rng.rand(M) < (1.0 if _ == 0 else 0.4))
        states[on, rng.randint(S, size=len(on)), rng.randint(S, size=len(on)), 8] = 1
    states[::4, :, :, 9:] = 0
    env, _, _ = make_env(2, seed=3, obs_mode='state', raster=raster, size=(S, S), max_steps=17)
    got = env.render_states(states).cpu().numpy().astype(np.int64)
    want = np.stack([ref(st.astype(np.int64)) for st in states])
    assert want.max() > 255 and tuple(got.shape) == (M,) + tuple(env.frame_shape)
    same('render_states', 0, got, want)
    for j in range(M - 3, M):
        assert np.array_equal(got[j], want[j]), 'state %d, in the second round of the loop' % j
    env.close()
