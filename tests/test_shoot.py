"""GPU tier of shooting plans: cw_shoot_kernel through CraftingWorldVecEnv.shoot, cw_shoot_actions_kernel through .shoot_actions.  The shared recipe is
checked row by row with shoot_check.check_shoot (itself tested on the CPU, tests/test_shoot_logic.py) against the numpy model of the draw and the CPU
oracle; every lane-group width and tail against simulate(shoot_actions(...)) on the device, reduced by the rule of craftingworld.h with torch; the plans
fed back through simulate(); the engine before and after every checked call byte for byte.  Everything is bit-exact.  No timing."""
import ctypes as C

import numpy as np
import pytest
import torch

from engines import ENGINES, K5, N1, k_of
from hostlib import host_lib
from masked_check import spread, take
from oracle_replay import make_env, np_states
from records_check import encode
from records_gpu import SENT, caller_records, dev as _dev, env_of_cases as _env_of, host, sentinel_out, walk_goals as _walk_goals, walked_engine
from shoot_check import FIELDS, LONG, RECIPE_KW, SHAPES, assert_coverage, check_shoot, coverage, layout, model_actions, recipe_shots

pytestmark = pytest.mark.gpu

_WIDTH = dict(best_ret=4, best_sample=4, best_action=1, length=4, done=1, achieved_mask=2, hdr=16, slot_pos=16, plan=1, ret=4)
_DTYPE = dict(best_ret=torch.int32, best_sample=torch.int32, best_action=torch.uint8, length=torch.int32, done=torch.bool, achieved_mask=torch.int16,
              hdr=torch.uint8, slot_pos=torch.int16, plan=torch.uint8, ret=torch.int32)
PER_PLAN = ('length', 'done', 'achieved_mask', 'hdr', 'slot_pos')      # what simulate() returns for a plan besides its return
KS = (1, 2, 3, 5, 8, 16, 33, 64, 100)


def _sentinel_out(T, K, M):
    """output buffers as shoot(out=...) takes them, every byte SENT"""
    return sentinel_out(layout(T, K), _WIDTH, _DTYPE, M)


def _host(r):
    return host(r, FIELDS)


def _lanes(M, K):
    return host_lib()[1].cwh_shoot_lanes_of(M, K)


def _via_simulate(env, T, K, seed, hdr, pos, env_of=None, weights=None):
    """the same results the long way round, on the device: the whole action tensor (shoot_actions), simulate(stop_at_done=True) of all K samples of every
    record, reduced by the rule of craftingworld.h -- the maximum, the smallest sample that reaches it (no argmax, whose ties are not pinned) -> the ten fields"""
    M = hdr.shape[0]
    acts = env.shoot_actions(T, seed, rows=K, weights=weights, n_states=M)
    assert tuple(acts.shape) == (T, K, M) and acts.dtype == torch.uint8
    eo = (torch.arange(M, device='cuda', dtype=torch.int32) % env.num_envs) if env_of is None else env_of
    r = env.simulate(acts.view(T, K * M), hdr.repeat(K, 1), pos.repeat(K, 1), eo.repeat(K))
    ret = r['ret'].view(K, M)
    best = ret.amax(dim=0)
    first = torch.where(ret == best[None], torch.arange(K, device='cuda')[:, None], K).amin(dim=0)
    cols = torch.arange(M, device='cuda')
    out = {f: r[f][first * M + cols] for f in PER_PLAN}
    out.update(best_ret=best, best_sample=first.to(torch.int32), plan=acts[:, first, cols].contiguous(), ret=ret.contiguous())
    out['best_action'] = out['plan'][0]
    return out


# ------------------------------------------------------------------------------------------------------------------------------ 1. the shared recipe
@pytest.mark.parametrize('style', [None, 'subset'])
@pytest.mark.parametrize('shape', SHAPES + (LONG,), ids=lambda s: 'T%d_K%d_seed%d' % s)
def test_the_recipe_against_the_oracle(shape, style):
    """600 records -- two full workgroups and a tail -- handed in through hdr= / slot_pos= / env_of=; all ten fields into sentinel-filled buffers, under
    both reward rules; what the shape exercises is asserted from the oracle alone before anything is compared"""
    T, K, seed = shape
    dense, init_grids, want = recipe_shots(T, K, seed, style, 24 if shape == LONG else 12)
    cov = coverage(want, T, RECIPE_KW['max_steps'])
    none = ~want['any_success']
    if shape == LONG:                                                             # the horizon passes max_steps: no success means the time-out at step 17
        assert cov['timeout'] >= 200 and none.sum() == cov['timeout'] and want['done'][none].all()
        assert (want['length'][none] == 17).all() and (want['best_ret'][none] == -17).all()
    else:
        assert_coverage(cov)
        assert (want['best_sample'][none] == 0).all()
    M = len(dense['hold'])
    env, _, _ = make_env(M, *np_states(M, 900), obs_mode='state', reward_style=style, auto_reset=False, **RECIPE_KW)
    env.reset()
    before = take(env)
    assert np.array_equal(before['state_init_grid'], init_grids)                  # (env j's episode is oracle env j's: it supplies the start positions)
    hdr, pos = encode(dense, menu=before['hdr'][:, 3])
    env_of = np.arange(M)
    out = _sentinel_out(T, K, M)
    r = env.shoot(T, K, seed, _dev(hdr), _dev(pos.view(np.int16), np.int16), _dev(env_of, np.int32), fields=FIELDS, out=out)
    assert all(r[f] is out[f] for f in FIELDS)
    part, skipped = check_shoot(before, take(env), dict(hdr=hdr, slot_pos=pos), env_of, T, K, seed, None, _host(out), SENT, oracle_kw=RECIPE_KW,
                                expected=(dense, want))
    assert (part, skipped) == (M, 0)
    env.close()


def test_every_winning_length_occurs():
    lengths = {6: set(), 12: set()}
    for T, K, seed in SHAPES:
        lengths[T] |= set(coverage(recipe_shots(T, K, seed, None, 12)[2], T, RECIPE_KW['max_steps'])['lengths'])
    assert lengths[6] >= set(range(1, 6)) and lengths[12] >= set(range(1, 12))


# ------------------------------------------------------------------------------------------------------------------------------ 2. every lane-group width and tail
@pytest.fixture(scope='module')
def engine70():
    env = walked_engine(87000, 9, goals=(2, 88))
    yield env
    env.close()


def _records(before, e, M):
    return caller_records(before, e, M, N1, K5['max_steps'])


def test_the_shapes_hit_every_width():
    got = {_lanes(M, K) for M in (600, 65, 1) for K in KS} | {_lanes(65536, 4)}
    assert got == {1, 2, 4, 8, 16, 32, 64} and _lanes(65536, 4) == 1 and _lanes(600, 64) == 64 and _lanes(1, 100) == 64


@pytest.mark.parametrize('weighted', [False, True], ids=['uniform', 'weighted'])
@pytest.mark.parametrize('M', [600, 65, 1])
@pytest.mark.parametrize('K', KS)
def test_lane_groups_against_simulate(engine70, K, M, weighted):
    """K samples on G = 1 .. 64 lanes a state, K a multiple of G and not (the tail round of the sample loop), T = 6: one block of weights and a tail of two"""
    env, T, seed = engine70, 6, 1000 + K
    before = take(env)
    e = np.arange(M) % N1
    hdr, pos = _records(before, e, M)
    hdr, pos, eo = _dev(hdr), _dev(pos, np.int16), _dev(e, np.int32)
    w = None
    if weighted:
        w = np.random.RandomState(K).randint(0, 4, (T, 6, M)) * np.random.RandomState(K + 1).randint(1, 16384, (T, 6, M))
        w = torch.as_tensor(w.astype(np.uint16), device='cuda')
    want = _via_simulate(env, T, K, seed, hdr, pos, eo, w)
    out = _sentinel_out(T, K, M)
    env.shoot(T, K, seed, hdr, pos, eo, weights=w, fields=FIELDS, out=out)
    for f in FIELDS:
        assert torch.equal(out[f], want[f]), (K, M, f)
    after = take(env)
    assert all(np.array_equal(before[k], after[k]) for k in before)
    if M == 600 and K >= 8:
        ok = want['done'] & (want['best_ret'] > 0)
        assert ok.sum() >= 20 and (~ok).sum() >= 20 and (want['best_sample'] > 0).sum() >= 20


@pytest.mark.parametrize('weighted', [False, True], ids=['uniform', 'weighted'])
def test_one_lane_a_state_with_several_samples(engine70, weighted):
    """M = 65 536, K = 4, T = 4: G = 1, every lane plays all four samples"""
    env, M, K, T, seed = engine70, 65536, 4, 4, 77
    e = np.arange(M) % N1
    hdr, pos = _records(take(env), e, M)
    hdr, pos, eo = _dev(hdr), _dev(pos, np.int16), _dev(e, np.int32)
    w = torch.as_tensor((np.random.RandomState(5).randint(0, 3, (T, 6, M)) * 21845).astype(np.uint16), device='cuda') if weighted else None
    want = _via_simulate(env, T, K, seed, hdr, pos, eo, w)
    got = env.shoot(T, K, seed, hdr, pos, eo, weights=w, fields=FIELDS)
    for f in FIELDS:
        assert torch.equal(got[f], want[f]), f


# ------------------------------------------------------------------------------------------------------------------------------ 3. env_of
@pytest.mark.parametrize('M,K,T', [(63, 5, 3), (257, 64, 4), (1000, 8, 2)])
def test_env_of_on_the_device(engine70, M, K, T):
    """env_of handed over as a device tensor: random envs with repeats, -1 and -7 (no part: sentinel rows in all ten fields, ret and plan columns included),
    N, N + 31 and INT32_MAX (skipped, and counted once each -- not once per lane: at M = 257, K = 64 a state has 64 of them)"""
    env, seed = engine70, 5
    assert _lanes(257, 64) == 64
    e = _env_of(M, N1)
    before = take(env)
    hdr, pos = _records(before, e, M)
    out = _sentinel_out(T, K, M)
    skipped0 = env.expand_skipped
    env.shoot(T, K, seed, _dev(hdr), _dev(pos, np.int16), _dev(e, np.int32), fields=FIELDS, out=out)
    part, skipped = check_shoot(before, take(env), dict(hdr=hdr, slot_pos=pos), e, T, K, seed, None, _host(out), SENT, oracle_kw=K5)
    assert skipped == int((e >= N1).sum()) >= 2 and part == int(((e >= 0) & (e < N1)).sum()) and (e < 0).sum() >= 2
    assert env.expand_skipped == skipped0 + skipped
    with pytest.raises(IndexError):                                               # the host-validated path refuses what the kernel skips
        env.shoot(T, K, seed, hdr, pos, e)
    if M == 63:                                                                   # every single field: the other buffers stay as they were
        for f in FIELDS:
            bufs = _sentinel_out(T, K, M)
            before = take(env)
            r = env.shoot(T, K, seed, _dev(hdr), _dev(pos, np.int16), _dev(e, np.int32), fields=[f], out={f: bufs[f]})
            assert list(r) == [f]
            check_shoot(before, take(env), dict(hdr=hdr, slot_pos=pos), e, T, K, seed, None, _host(r), SENT, oracle_kw=K5)
            assert all(bool((bufs[g].view(torch.uint8) == SENT).all()) for g in FIELDS if g != f), f


# ------------------------------------------------------------------------------------------------------------------------------ 4. weights
def _weights(kind, T, M):
    rng = np.random.RandomState(31)
    if kind == 'random':
        return rng.randint(0, 65536, (T, 6, M))
    if kind == 'forbidden':                                                       # one action per state never drawn
        w = rng.randint(1, 1000, (T, 6, M))
        w[:, np.arange(M) % 6, np.arange(M)] = 0
        return w
    if kind == 'zero_rows':                                                       # W == 0 at every third (step, state): uniform there
        w = rng.randint(0, 50, (T, 6, M))
        w[:, :, ::3] *= (np.arange(T) % 2)[:, None, None]
        return w
    if kind == 'all_65535':
        return np.full((T, 6, M), 65535)
    return rng.randint(0, 9, (T, 6))                                              # 'broadcast': [T, 6]


@pytest.mark.parametrize('kind', ['random', 'forbidden', 'zero_rows', 'all_65535', 'broadcast'])
def test_weights(engine70, kind):
    env, T, K, M, seed = engine70, 12, 33, 200, 2 ** 63 + 11
    before = take(env)
    e = np.arange(M) % N1
    hdr, pos = _records(before, e, M)
    w = _weights(kind, T, M)
    full = np.broadcast_to(w[:, :, None], (T, 6, M)) if w.ndim == 2 else w
    given = torch.as_tensor(w.astype(np.uint16), device='cuda') if kind in ('random', 'broadcast') else w          # in place / broadcast on the device / the host path
    out = _sentinel_out(T, K, M)
    env.shoot(T, K, seed, _dev(hdr), _dev(pos, np.int16), _dev(e, np.int32), weights=given, fields=FIELDS, out=out)
    check_shoot(before, take(env), dict(hdr=hdr, slot_pos=pos), e, T, K, seed, full, _host(out), SENT, oracle_kw=K5)
    acts = env.shoot_actions(T, seed, rows=K, weights=given, n_states=M).cpu().numpy()
    assert np.array_equal(acts, model_actions(seed, M, K, T, full))
    if kind == 'forbidden':
        assert not (acts == (np.arange(M) % 6)[None, None, :]).any()
    if kind == 'all_65535':
        assert np.array_equal(acts, model_actions(seed, M, K, T))                 # equal weights are the uniform draw


# ------------------------------------------------------------------------------------------------------------------------------ 5. shoot_actions
def test_shoot_actions(engine70):
    env, T, K, M, seed = engine70, 9, 37, 333, 0xDEADBEEF12345678
    acts = env.shoot_actions(T, seed, rows=K, n_states=M)
    assert np.array_equal(acts.cpu().numpy(), model_actions(seed, M, K, T))
    own = env.shoot_actions(T, seed, rows=3)                                      # n_states defaults to num_envs
    assert torch.equal(own, acts[:, :3, :N1])
    e = np.arange(M) % N1
    hdr, pos = _records(take(env), e, M)
    hdr, pos, eo = _dev(hdr), _dev(pos, np.int16), _dev(e, np.int32)
    r = env.shoot(T, K, seed, hdr, pos, eo, fields=FIELDS)
    assert torch.equal(env.shoot_actions(T, seed, samples=r['best_sample'][None], n_states=M)[:, 0], r['plan'])
    s = np.random.RandomState(4).randint(-3, 65536, (5, M))
    s[0, :7] = [-1, 0, 65535, -2 ** 31, 2 ** 31 - 1, 1, -7]
    s[2, ::9] = -5
    out = torch.full((T, 5, M), SENT, dtype=torch.uint8, device='cuda')
    assert env.shoot_actions(T, seed, samples=_dev(s, np.int32), n_states=M, out=out) is out
    want = model_actions(seed, M, K, T, samples=s)
    assert (s < 0).sum() >= 10 and np.array_equal(out.cpu().numpy(), np.where(want < 0, SENT, want))
    assert np.array_equal(env.shoot_actions(T, seed, samples=s, n_states=M).cpu().numpy()[:, s >= 0], want[:, s >= 0])      # (the host path)
    back = env.simulate(r['plan'], hdr, pos, eo, stop_at_done=True)              # the plan IS an action tensor of simulate()
    assert torch.equal(back['ret'], r['best_ret'])
    for f in PER_PLAN:
        assert torch.equal(back[f], r[f]), f
    assert (r['length'] < T).any() and torch.equal(r['best_action'], r['plan'][0])


# ------------------------------------------------------------------------------------------------------------------------------ 6. the seed word
def test_seed_dev(engine70):
    env, T, K, M = engine70, 5, 16, N1
    for value in (0, 12345, 2 ** 63 + 9, 2 ** 64 - 1):
        want = env.shoot(T, K, value, fields=FIELDS)
        for dtype in (torch.uint64, torch.int64):
            word = torch.tensor([value if dtype is torch.uint64 or value < 2 ** 63 else value - 2 ** 64], dtype=dtype, device='cuda')
            got = env.shoot(T, K, word, fields=FIELDS)
            for f in FIELDS:
                assert torch.equal(got[f], want[f]), (value, f)
            assert torch.equal(env.shoot_actions(T, word, rows=K), env.shoot_actions(T, value, rows=K))
    from gym_craftingworld_amd import _lib as L
    lib, h, st = env._lib, env._h, env._stream()
    for a, b in ((3, 4), (2 ** 64 - 3, 10), (2 ** 63, 2 ** 63), (2 ** 64 - 1, 2 ** 64 - 1)):               # seed = a + b mod 2^64: the wrap included
        word = torch.tensor([b], dtype=torch.uint64, device='cuda')
        out = _sentinel_out(T, K, M)
        struct = L.cw_shoot_out(**{('achieved' if f == 'achieved_mask' else f): t.data_ptr() for f, t in out.items()})
        assert lib.cw_shoot(h, None, None, None, M, T, K, a, C.c_void_p(word.data_ptr()), None, C.byref(struct), st) == L.CW_OK
        want = env.shoot(T, K, (a + b) % 2 ** 64, fields=FIELDS)
        for f in FIELDS:
            assert torch.equal(out[f], want[f]), (a, b, f)
        acts = torch.empty((T, K, M), dtype=torch.uint8, device='cuda')
        assert lib.cw_shoot_actions(h, M, T, a, C.c_void_p(word.data_ptr()), None, None, K, C.c_void_p(acts.data_ptr()), st) == L.CW_OK
        assert torch.equal(acts, env.shoot_actions(T, (a + b) % 2 ** 64, rows=K))
    assert not torch.equal(env.shoot_actions(T, 1, rows=K), env.shoot_actions(T, 1 << 32, rows=K))


# ------------------------------------------------------------------------------------------------------------------------------ 7. every engine kind
def _own_states(ekw, N, seed, okw=K5, steps=7, T=6, K=10):
    env, _, _ = make_env(N, *np_states(N, seed), **ekw, **okw)
    env.reset()
    spread(env, steps, 4)
    _walk_goals(env, 2, seed + 1)
    sn = env.get_state()['step_num'].copy()
    sn[::5] = okw['max_steps'] - 2                                # every fifth env two steps before the time-out
    env.set_state(step_num=sn)
    before = take(env)
    if env.obs_mode != 'state':
        assert 'observation' in before and 'desired_goal' in before
    r = env.shoot(T, K, seed, fields=FIELDS)
    part, skipped = check_shoot(before, take(env), None, None, T, K, seed, None, _host(r), SENT, oracle_kw=okw)      # (every buffer, stream, frame and counter: purity)
    assert (part, skipped) == (N, 0)
    assert r['done'].any() and not r['done'].all()
    env.close()


@pytest.mark.parametrize('engine', list(ENGINES))
def test_the_engines_own_states_on_every_engine(engine):
    _own_states(dict(ENGINES[engine]), N1, 91000)


def test_host_outputs_engine():
    """an engine whose outputs live in mapped host memory: the same call, synchronised on return"""
    _own_states(dict(obs_mode='pixels_dirty', host_outputs=True, auto_reset=False), 4, 92000)


def test_on_a_large_grid():
    """182 x 182, ten steps in: slot cells above 32 767 (negative in the int16 tensors)"""
    _own_states(dict(obs_mode='state', auto_reset=False), 9, 89000, okw=k_of(182), steps=10)


def test_no_states_and_bad_arguments_of_the_method(engine70):
    env = engine70
    r = env.shoot(5, 3, 0, hdr=torch.empty((0, 16), dtype=torch.uint8, device='cuda'), slot_pos=torch.empty((0, 8), dtype=torch.int16, device='cuda'), fields=FIELDS)
    assert set(r) == set(FIELDS) and tuple(r['plan'].shape) == (5, 0) and tuple(r['ret'].shape) == (3, 0)
    assert set(env.shoot(2, 2)) == {'best_ret', 'best_sample', 'best_action', 'length', 'done', 'achieved_mask', 'plan'}             # (the default fields)
    good = env.shoot(2, 4, fields=FIELDS)
    for bad in (dict(horizon=0), dict(samples=0), dict(samples=65537), dict(seed=-1), dict(seed=torch.zeros(1, dtype=torch.int64)), dict(fields=[]),
                dict(fields=['ret', 'frames']), dict(hdr=env.hdr), dict(env_of=torch.zeros(N1, dtype=torch.int32, device='cuda')), dict(out={'ret': good['ret']}),
                dict(out=dict(good, ret=good['ret'].to(torch.int64))), dict(out=dict(good, plan=good['plan'][:1])), dict(out=dict(good, done=good['done'].cpu())),
                dict(weights=torch.zeros((2, 6, N1 + 1), dtype=torch.uint16, device='cuda')), dict(horizon=3, out=good), dict(samples=5, out=good)):
        kw = dict(dict(horizon=2, samples=4, fields=FIELDS), **bad)
        with pytest.raises(ValueError):
            env.shoot(kw.pop('horizon'), kw.pop('samples'), **kw)
    with pytest.raises(TypeError):
        env.shoot(2, 4, weights=torch.ones((2, 6, N1), device='cuda'))


# ------------------------------------------------------------------------------------------------------------------------------ 8. the entry points
def test_errors_of_the_entry_points():
    from gym_craftingworld_amd import CraftingWorldVecEnv, _lib as L
    N, T, K = 8, 3, 4
    env = CraftingWorldVecEnv(N, obs_mode='state', auto_reset=False, seed=3, **K5)
    lib, h, st = env._lib, env._h, env._stream()
    bufs = _sentinel_out(T, K, N)
    vp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    one = lambda **kw: L.cw_shoot_out(**kw)  # noqa: E731
    full = one(**{('achieved' if f == 'achieved_mask' else f): vp(t) for f, t in bufs.items()})
    acts = torch.full((T, K, N), SENT, dtype=torch.uint8, device='cuda')
    with pytest.raises(L.CraftingWorldError):                                      # before reset(), through the methods
        env.shoot(T, K)
    with pytest.raises(L.CraftingWorldError):
        env.shoot_actions(T, rows=K)
    assert lib.cw_shoot(h, None, None, None, N, T, K, 0, None, None, C.byref(full), st) == L.CW_ERR_STATE and b'before cw_reset' in lib.cw_last_error()
    assert lib.cw_shoot_actions(h, N, T, 0, None, None, None, K, vp(acts), st) == L.CW_ERR_STATE and b'before cw_reset' in lib.cw_last_error()
    env.reset()
    ch, cp, eo = env.hdr.clone(), env.slot_pos.clone(), vp(torch.zeros(N, dtype=torch.int32, device='cuda'))
    w = torch.ones((T, 6, N), dtype=torch.uint16, device='cuda')
    assert lib.cw_shoot(h, None, None, None, N, T, K, 0, None, None, C.byref(full), st) == L.CW_OK
    assert lib.cw_shoot(h, None, None, None, N, T, K, 0, None, vp(w), C.byref(full), st) == L.CW_OK
    torch.cuda.synchronize()
    assert all(not bool((t.view(torch.uint8) == SENT).all()) for t in bufs.values())
    assert lib.cw_shoot(h, None, vp(ch), vp(cp), 0, T, K, 0, None, None, C.byref(full), st) == L.CW_OK      # no states: nothing enqueued
    assert lib.cw_shoot_actions(h, 0, T, 0, None, None, None, K, vp(acts), st) == L.CW_OK
    assert lib.cw_shoot_actions(h, N, T, 0, None, None, None, 0, vp(acts), st) == L.CW_OK
    torch.cuda.synchronize()
    assert bool((acts == SENT).all())
    big = torch.zeros(16 * N * 3, dtype=torch.uint8, device='cuda')              # hdr | slot_pos | room: outputs that overlap the records read
    big[:16 * N].copy_(ch.view(-1))
    big[16 * N:32 * N].copy_(cp.view(torch.uint8).view(-1))
    invalid = [((None, None, None, None, N, T, K, 0, None, None, C.byref(full)), b'engine'),
               ((h, None, None, None, N, T, K, 0, None, None, None), b'out'),
               ((h, None, None, None, N, T, K, 0, None, None, C.byref(one())), b'every field'),
               ((h, None, vp(ch), vp(cp), -1, T, K, 0, None, None, C.byref(full)), b'n_states'),
               ((h, None, vp(ch), vp(cp), 2 ** 27 + 1, T, K, 0, None, None, C.byref(full)), b'n_states'),
               ((h, None, None, None, N, 0, K, 0, None, None, C.byref(full)), b'n_steps'),
               ((h, None, None, None, N, 32768, K, 0, None, None, C.byref(full)), b'n_steps'),
               ((h, None, None, None, N, T, 0, 0, None, None, C.byref(full)), b'n_samples'),
               ((h, None, None, None, N, T, 65537, 0, None, None, C.byref(full)), b'n_samples'),
               ((h, None, vp(ch), vp(cp), 65537, 64, 1024, 0, None, None, C.byref(full)), b'above 2^32'),
               ((h, None, vp(ch), vp(cp), 65536, 65, 1024, 0, None, None, C.byref(full)), b'above 2^32'),
               ((h, None, None, None, N - 1, T, K, 0, None, None, C.byref(full)), b'must be num_envs'),
               ((h, None, None, None, 2 * N, T, K, 0, None, None, C.byref(full)), b'must be num_envs'),
               ((h, None, vp(ch), None, N, T, K, 0, None, None, C.byref(full)), b'hdr_in given without slot_pos_in'),
               ((h, None, None, vp(cp), N, T, K, 0, None, None, C.byref(full)), b'slot_pos_in given without hdr_in'),
               ((h, eo, None, None, N, T, K, 0, None, None, C.byref(full)), b'env_of'),
               ((h, None, vp(ch, 8), vp(cp), N - 1, T, K, 0, None, None, C.byref(full)), b'hdr_in is not 16-byte aligned'),
               ((h, None, vp(ch), vp(cp, 2), N - 1, T, K, 0, None, None, C.byref(full)), b'slot_pos_in is not 16-byte aligned'),
               ((h, None, vp(ch), vp(cp), N - 1, T, K, 0, None, None, C.byref(one(hdr=vp(bufs['hdr'], 4)))), b'out->hdr is not 16-byte aligned'),
               ((h, None, vp(ch), vp(cp), N - 1, T, K, 0, None, None, C.byref(one(ret=vp(bufs['ret']), slot_pos=vp(bufs['slot_pos'], 8)))), b'out->slot_pos is not 16-byte aligned'),
               ((h, None, vp(big), vp(big, 16 * N), N, T, K, 0, None, None, C.byref(one(hdr=vp(big, 16 * (N - 1))))), b'out->hdr overlaps the records'),
               ((h, None, vp(big), vp(big, 16 * N), N, T, K, 0, None, None, C.byref(one(slot_pos=vp(big, 16 * (2 * N - 1))))), b'out->slot_pos overlaps the records'),
               ((h, None, vp(big), vp(big, 16 * N), N, T, K, 0, None, None, C.byref(one(plan=vp(big, 16 * N - 1)))), b'out->plan overlaps the records'),
               ((h, None, vp(big), vp(big, 16 * N), N, T, K, 0, None, None, C.byref(one(ret=vp(big, 32 * N - 4)))), b'out->ret overlaps the records'),
               ((h, None, None, None, N, T, K, 0, None, vp(w), C.byref(one(plan=vp(w, 12 * T * N - 1)))), b'out->plan overlaps the weights'),
               ((h, None, None, None, N, T, K, 0, None, vp(w), C.byref(one(ret=vp(w)))), b'out->ret overlaps the weights'),
               ((h, None, None, None, N, T, K, 0, None, None, C.byref(one(hdr=vp(env.hdr)))), b'out->hdr overlaps the records')]
    for args, word in invalid:
        assert lib.cw_shoot(*args, st) == L.CW_ERR_INVALID, word
        assert word in lib.cw_last_error(), (word, lib.cw_last_error())
    assert lib.cw_shoot(h, None, vp(big), vp(big, 16 * N), N, T, K, 0, None, None, C.byref(one(plan=vp(big, 32 * N))), st) == L.CW_OK       # (adjacent is not overlapping)
    invalid = [((None, N, T, 0, None, None, None, K, vp(acts)), b'engine'), ((h, N, T, 0, None, None, None, K, None), b'out'),
               ((h, -1, T, 0, None, None, None, K, vp(acts)), b'n_states'), ((h, 2 ** 27 + 1, T, 0, None, None, None, K, vp(acts)), b'n_states'),
               ((h, N, T, 0, None, None, None, -1, vp(acts)), b'n_rows'), ((h, N, T, 0, None, None, None, 2 ** 27 + 1, vp(acts)), b'n_rows'),
               ((h, N, 0, 0, None, None, None, K, vp(acts)), b'n_steps'), ((h, N, 32768, 0, None, None, None, K, vp(acts)), b'n_steps'),
               ((h, 65537, 64, 0, None, None, None, 1024, vp(acts)), b'above 2^32'), ((h, 2 ** 27, 1, 0, None, None, None, 2 ** 27, vp(acts)), b'above 2^32')]
    for args, word in invalid:
        assert lib.cw_shoot_actions(*args, st) == L.CW_ERR_INVALID, word
        assert word in lib.cw_last_error(), (word, lib.cw_last_error())
    torch.cuda.synchronize()
    assert env.expand_skipped == 0
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 9. capture
def test_captured_into_a_graph_with_a_step():
    """torch.cuda.graph around step(actions) + shoot(out=..., seed=tensor): the calls only enqueue; each replay steps the env and shoots from the state it
    reaches with the seed the word then holds, equal to the eager calls with that seed on a twin engine in the same state"""
    N, T, K = 300, 6, 20
    env, keys, pos = make_env(N, *np_states(N, 93000), obs_mode='state', auto_reset=False, **K5)
    twin, _, _ = make_env(N, keys, pos, obs_mode='state', auto_reset=False, **K5)
    for e in (env, twin):
        e.reset()
        spread(e, 5, 6)
        _walk_goals(e, 3, 94)
    assert torch.equal(env.hdr, twin.hdr) and torch.equal(env.slot_pos, twin.slot_pos)
    acts = _dev(np.random.RandomState(95).randint(0, 6, N))
    word = torch.tensor([2 ** 64 - 2], dtype=torch.uint64, device='cuda')
    out = _sentinel_out(T, K, N)
    env.shoot(T, K, word, fields=FIELDS)                                          # (warm-up outside the capture)
    env.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.step_async(acts)
        env.shoot(T, K, word, fields=FIELDS, out=out)
    assert all(bool((t.view(torch.uint8) == SENT).all()) for t in out.values())          # (capturing ran nothing)
    plans = []
    for rnd, value in enumerate((2 ** 64 - 2, 2 ** 64 - 1, 0)):                    # the word bumped between the replays, past the wrap
        acts.copy_(_dev(np.random.RandomState(96 + rnd).randint(0, 6, N)))
        word.copy_(torch.tensor([value], dtype=torch.uint64))
        g.replay()
        twin.step(acts)
        eager = twin.shoot(T, K, value, fields=FIELDS)
        for f in FIELDS:
            assert torch.equal(out[f], eager[f]), (rnd, f)
        assert torch.equal(env.hdr, twin.hdr)
        plans.append(out['plan'].clone())
    assert not torch.equal(plans[0], plans[1]) and not torch.equal(plans[1], plans[2])
    torch.cuda.synchronize()
    env.close()
    twin.close()
