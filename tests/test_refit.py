"""GPU tier of the refit: cw_refit_select_kernel and cw_refit_count_kernel through CraftingWorldVecEnv.shoot_refit, and .cem on top of them.  Every call is
checked with refit_check.check_refit (itself tested on the CPU, tests/test_refit_logic.py) against the numpy model written from the header: every lane-group
width, tail and round of the selection on six kinds of returns, the counts uniform and weighted, separate and in place, the clamp, the states that take
no part, every engine kind, the entry point's errors, and cem() against the hand-written loop, the oracle and a captured graph.  Everything is bit-exact.
No timing."""
import ctypes as C

import numpy as np
import pytest
import torch

import refit_check as rc
from engines import ENGINES, K5, N1, n_cu
from hostlib import host_lib
from masked_check import spread, take
from oracle_replay import make_env, np_states
from records_check import encode
from records_gpu import dev as _dev, env_of_cases as _env_of, walk_goals as _walk_goals, walked_engine
from shoot_check import RECIPE_KW, expected_shoot, recipe_shots
from simulate_check import recipe

pytestmark = pytest.mark.gpu

FIELDS = rc.FIELDS
MS, KS = (1, 65, 600), (1, 2, 5, 9, 17, 63, 64, 65, 100, 129, 1000)      # (9 and 17: the widths 8 and 16, each with a tail)
SENT = dict(elites=-99, weights=0xABCD, elite_min=-98)
_NP = dict(elites=np.int32, weights=np.uint16, elite_min=np.int32)


def elite_counts(K):
    return sorted({1, -(-K // 3), K})


def _lanes(M, K):
    return host_lib()[1].cwh_shoot_lanes_of(M, K)


def _sentinel_out(T, E, M, fields=FIELDS):
    shape = dict(elites=(E, M), weights=(T, 6, M), elite_min=(M,))
    return {f: _dev(np.full(shape[f], SENT[f], _NP[f]), _NP[f]) for f in fields}


def _np(d):
    return {f: t.cpu().numpy() for f, t in d.items()}


def refit(env, ret, E, T, seed, weights=None, env_of=None, smooth=1, gain=1, in_place=False, fields=FIELDS, want=None):
    """one shoot_refit call on numpy inputs, into sentinel-filled buffers (in place: into the weights' own), checked by check_refit -> the outputs as numpy"""
    ret_d = _dev(ret, np.int32)
    w_d = None if weights is None else _dev(weights, np.uint16)
    e_d = None if env_of is None else _dev(env_of, np.int32)
    out = _sentinel_out(T, E, ret.shape[1], fields)
    if in_place:
        out['weights'] = w_d
    before = _np(out)
    r = env.shoot_refit(ret_d, E, T, seed, weights=w_d, env_of=e_d, smooth=smooth, gain=gain, fields=fields, out=out)
    assert all(r[f] is out[f] for f in fields)
    after = _np(out)
    rc.check_refit(ret, ret_d.cpu().numpy(), weights, None if w_d is None or in_place else w_d.cpu().numpy(), env_of, env.num_envs, E, T, seed, smooth, gain,
                   before, after, in_place=in_place, want=want)
    return after


@pytest.fixture(scope='module')
def engine70():
    env = walked_engine(87000, 9, goals=(2, 88))
    yield env
    env.close()


@pytest.fixture(scope='module')
def recipe_returns():
    """K -> the returns shoot() gives simulate_check.recipe(12)'s 600 states at T = 6, seed 3: int32 [K, 600] from the card (tests/test_shoot.py holds them
    against the oracle), computed once per K"""
    dense, init_grids, _ = recipe(12, None)
    M = len(dense['hold'])
    env, _, _ = make_env(M, *np_states(M, 900), obs_mode='state', auto_reset=False, **RECIPE_KW)
    env.reset()
    hdr, pos = encode(dense, menu=take(env)['hdr'][:, 3])
    hdr, pos, eo = _dev(hdr), _dev(pos.view(np.int16), np.int16), _dev(np.arange(M), np.int32)
    held = {}

    def get(K):
        if K not in held:
            held[K] = env.shoot(6, K, 3, hdr, pos, eo, fields=('ret',))['ret'].cpu().numpy()
        return held[K]
    yield get
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 1. the selection
def test_the_shapes_hit_every_width():
    got = {_lanes(M, K) for M in MS for K in KS} | {_lanes(65536, 4)}
    assert got == {1, 2, 4, 8, 16, 32, 64} and _lanes(65536, 4) == 1 and _lanes(600, 63) == 32 and _lanes(1, 1000) == 64 and _lanes(600, 1000) == 64
    assert -(-1000 // 64) == 16 and -(-129 // 64) == 3                            # more than one round a lane, and a tail round


@pytest.mark.parametrize('K', KS)
@pytest.mark.parametrize('M', MS)
@pytest.mark.parametrize('kind', ('shoot',) + rc.KINDS)
def test_selection(engine70, recipe_returns, kind, M, K):
    """E = 1, a third, all of K samples on G = 1 .. 64 lanes a state; where a sample is left unchosen, every tie-bearing kind has a state whose threshold value
    is held by a chosen and an unchosen sample (asserted from the model before the call)"""
    for E in elite_counts(K):
        if kind == 'shoot':
            full = recipe_returns(K)
            ret = np.ascontiguousarray(full[:, rc.shoot_columns(full, M, E)])
        else:
            ret = rc.columns(kind, K, M, E)
        if K > E and kind in ('shoot',) + rc.TIE_BEARING:
            assert rc.split_ties(ret, E).any(), (kind, M, K, E)
        got = refit(engine70, ret, E, 2, 1000 + K)
        assert got['elite_min'].min() >= ret.min() and (np.diff(got['elites'], axis=0) > 0).all()


@pytest.mark.parametrize('kind', ['two', 'perm', 'extremes'])
def test_one_lane_a_state(engine70, kind):
    """M = 65 536, K = 4, E = 2: G = 1, the lanes of a wave are 64 consecutive states"""
    ret = rc.columns(kind, 4, 65536, 2)
    assert _lanes(65536, 4) == 1 and (kind == 'perm' or rc.split_ties(ret, 2).sum() > 10000)
    refit(engine70, ret, 2, 3, 7)


def test_a_second_grid_stride_round_of_each_kernel(engine70):
    """both kernels are launched with at most cwh_refit_grid workgroups of 256 lanes; M_SECOND_ROUND states at K = 2 (G = 1: a lane a state) and T = 1 (a
    lane a state in the count kernel too) are 300 more than one round of either covers"""
    L, lib = host_lib()
    one_round = 256 * n_cu() * L.CWH_REFIT_BLOCKS_PER_CU
    M_SECOND_ROUND = one_round + 300
    assert lib.cwh_refit_grid_of(M_SECOND_ROUND, n_cu()) * 256 == one_round < M_SECOND_ROUND and _lanes(M_SECOND_ROUND, 2) == 1
    ret = rc.columns('two', 2, M_SECOND_ROUND, 1)
    assert rc.split_ties(ret[:, one_round:], 1).any()
    w = np.random.RandomState(2).randint(0, 3, (1, 6, M_SECOND_ROUND)) * 1000
    got = refit(engine70, ret, 1, 1, 5, weights=w)
    assert len(np.unique(got['elites'][0, one_round:])) == 2 and len(np.unique(got['weights'][:, :, one_round:])) == 2


# ------------------------------------------------------------------------------------------------------------------------------ 2. counts and weights
def _weights(T, M, seed):
    """[T, 6, M]: forbidden actions, whole rows of zeros (uniform there) and weights up to 49 149"""
    w = np.random.RandomState(seed).randint(0, 4, (T, 6, M)) * np.random.RandomState(seed + 1).randint(1, 16384, (T, 6, M))
    w[:, :, 7::50] = 0
    return w


@pytest.mark.parametrize('smooth', [0, 1])
@pytest.mark.parametrize('weighted', [False, True], ids=['uniform', 'weighted'])
@pytest.mark.parametrize('T', [1, 6, 24, 33])
def test_counts_and_weights(engine70, T, weighted, smooth):
    """the real returns of shoot() with the same seed and weights, refitted into a buffer of its own and in place: byte for byte the same"""
    env, M, K, E, seed, gain = engine70, 200, 33, 8, 2 ** 63 + T, 3
    w = _weights(T, M, T) if weighted else None
    if weighted:
        assert (w.sum(axis=1) == 0).any() and (w == 0).sum() > T * M
    e = np.arange(M) % N1
    before = take(env)
    hdr, pos = before['hdr'][e], before['slot_pos'][e]
    ret = env.shoot(T, K, seed, _dev(hdr), _dev(pos, np.int16), _dev(e, np.int32), weights=None if w is None else _dev(w, np.uint16),
                    fields=('ret',))['ret'].cpu().numpy()
    want = rc.expected_refit(ret, E, T, seed, w, smooth, gain)
    assert (want['counts'] == 0).any() and (smooth > 0 or (want['weights'] == 0).any())          # smooth = 0 forbids what no elite drew
    apart = refit(env, ret, E, T, seed, w, e, smooth, gain, want=want)
    if weighted:
        within = refit(env, ret, E, T, seed, w, e, smooth, gain, in_place=True, want=want)
        assert all(apart[f].tobytes() == within[f].tobytes() for f in FIELDS)
    after = take(env)
    assert all(np.array_equal(before[k], after[k]) for k in before)               # nothing of the engine is written


def test_the_clamp(engine70):
    """K = E = 100 with gain = 1 000: an action that 66 elites and more drew at a step is clamped to 65 535 -- weights that leave one action make it all 100"""
    M, K, T = 65, 100, 6
    w = np.random.RandomState(8).randint(1, 200, (T, 6, M))
    w[:, :, ::2] = 0
    w[:, np.arange(M) % 6, np.arange(M)] = 40000
    ret = rc.columns('perm', K, M, K)
    want = rc.expected_refit(ret, K, T, 9, w, 1, 1000)
    assert (want['counts'] == 100).any() and ((want['counts'] > 0) & (want['counts'] < 66)).any()
    assert (want['weights'] == 65535).any() and ((want['weights'] > 1) & (want['weights'] < 65535)).any()
    apart = refit(engine70, ret, K, T, 9, w, smooth=1, gain=1000, want=want)
    within = refit(engine70, ret, K, T, 9, w, smooth=1, gain=1000, in_place=True, want=want)
    assert apart['weights'].tobytes() == within['weights'].tobytes()


def test_all_samples_elite_is_the_histogram_of_the_draws(engine70):
    """no model at all: E = K, smooth = 0, gain = 1 and no weights_in -- the new weights are the histogram of shoot_actions(rows=K), counted in torch"""
    env, M, K, T, seed = engine70, 65536, 4, 6, 123456789
    ret = torch.zeros((K, M), dtype=torch.int32, device='cuda')
    r = env.shoot_refit(ret, K, T, seed, smooth=0, gain=1)
    acts = env.shoot_actions(T, seed, rows=K, n_states=M)
    hist = torch.stack([(acts == a).sum(dim=1) for a in range(6)], dim=1)
    assert tuple(hist.shape) == (T, 6, M) and torch.equal(r['weights'].view(torch.int16), hist.to(torch.int16))
    assert torch.equal(r['elites'], torch.arange(K, device='cuda', dtype=torch.int32)[:, None].expand(K, M)) and not r['elite_min'].any()


# ------------------------------------------------------------------------------------------------------------------------------ 3. states that take no part
@pytest.mark.parametrize('M,K,E,T', [(63, 5, 2, 3), (257, 64, 5, 4), (1000, 8, 3, 2)])
def test_env_of_on_the_device(engine70, M, K, E, T):
    """env_of handed over as a device tensor with -1, -7 (no part) and N, N + 31, INT32_MAX (the states cw_shoot skipped and counted): their rows stay as
    they were in all three outputs -- in place, the weights read --, and expand_skipped does not move"""
    env, seed = engine70, 5
    e = _env_of(M, N1)
    assert (e < 0).sum() >= 2 and (e >= N1).sum() >= 2 and _lanes(257, 64) == 64
    ret = np.random.RandomState(M).randint(-3, 3, (K, M)).astype(np.int32)
    w = _weights(T, M, M)
    skipped0 = env.expand_skipped
    before = take(env)
    refit(env, ret, E, T, seed, None, e)
    refit(env, ret, E, T, seed, w, e)
    refit(env, ret, E, T, seed, w, e, in_place=True)
    refit(env, ret, E, T, seed, None, e, fields=('elites',))
    refit(env, ret, E, T, seed, None, e, fields=('elites', 'elite_min'))
    got = refit(env, ret, E, T, seed, w, e, fields=('weights',))                  # (the elites go to a buffer of the env's own)
    assert list(got) == ['weights']
    assert env.expand_skipped == skipped0
    after = take(env)
    assert all(np.array_equal(before[k], after[k]) for k in before)
    with pytest.raises(IndexError):                                               # the host-validated path refuses what the kernel leaves out
        env.shoot_refit(_dev(ret, np.int32), E, T, seed, env_of=e)
    host = np.where(e >= N1, -1, e)                                               # ... and packs the rest as the records calls do
    r = env.shoot_refit(_dev(ret, np.int32), E, T, seed, env_of=host.tolist())
    part = rc.takes_part(e, N1, M)
    assert np.array_equal(r['weights'].cpu().numpy()[:, :, part], rc.expected_refit(ret, E, T, seed)['weights'][:, :, part])


# ------------------------------------------------------------------------------------------------------------------------------ 4. every engine kind
def _own_states(ekw, N, seed, T=6, K=10, E=3):
    env, _, _ = make_env(N, *np_states(N, seed), **ekw, **K5)
    env.reset()
    spread(env, 7, 4)
    _walk_goals(env, 2, seed + 1)
    r = env.shoot(T, K, seed, fields=('ret', 'best_ret'))
    before = take(env)
    ret = r['ret'].cpu().numpy() if not env.host_outputs else r['ret'].cpu().numpy().copy()
    got = refit(env, ret, E, T, seed)
    after = take(env)
    assert all(np.array_equal(before[k], after[k]) for k in before)               # every buffer, stream, frame and counter: purity
    assert np.array_equal(got['elite_min'] <= r['best_ret'].cpu().numpy(), np.ones(N, bool))
    env.close()


@pytest.mark.parametrize('engine', list(ENGINES))
def test_on_every_engine(engine):
    _own_states(dict(ENGINES[engine]), N1, 91000)


def test_host_outputs_engine():
    _own_states(dict(obs_mode='pixels_dirty', host_outputs=True, auto_reset=False), 4, 92000)


# ------------------------------------------------------------------------------------------------------------------------------ 5. the entry point
def test_errors_of_the_entry_point():
    from gym_craftingworld_amd import CraftingWorldVecEnv, _lib as L
    N, T, K, E = 8, 3, 4, 2
    env = CraftingWorldVecEnv(N, obs_mode='state', auto_reset=False, seed=3, **K5)
    lib, h, st = env._lib, env._h, env._stream()
    bufs = _sentinel_out(T, E, N)
    vp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    one = lambda **kw: L.cw_refit_out(**kw)  # noqa: E731
    full = one(**{f: vp(t) for f, t in bufs.items()})
    ret = torch.zeros((K + E, N), dtype=torch.int32, device='cuda')               # (E spare rows behind the K the calls read)
    w = torch.ones((T + 1, 6, N), dtype=torch.uint16, device='cuda')
    eo = torch.zeros(N + 1, dtype=torch.int32, device='cuda')
    with pytest.raises(L.CraftingWorldError):                                      # before reset(), through the method
        env.shoot_refit(ret[:K], E, T)
    assert lib.cw_shoot_refit(h, None, N, T, K, E, 0, None, None, vp(ret), 1, 1, C.byref(full), st) == L.CW_ERR_STATE and b'before cw_reset' in lib.cw_last_error()
    env.reset()
    assert lib.cw_shoot_refit(h, None, 0, T, K, E, 0, None, None, vp(ret), 1, 1, C.byref(full), st) == L.CW_OK       # no states: nothing enqueued
    torch.cuda.synchronize()
    assert all(bool((t == SENT[f]).all()) for f, t in _np(bufs).items())
    assert lib.cw_shoot_refit(h, vp(eo), N, T, K, E, 0, None, vp(w), vp(ret), 1, 1, C.byref(full), st) == L.CW_OK
    assert lib.cw_shoot_refit(h, None, N, T, K, E, 0, None, vp(w), vp(ret), 0, 65535, C.byref(one(elites=vp(bufs['elites']), weights=vp(w))), st) == L.CW_OK   # in place
    torch.cuda.synchronize()
    assert all(not bool((t == SENT[f]).all()) for f, t in _np(bufs).items())
    a = (h, None, N, T, K, E, 0, None, None, vp(ret), 1, 1, C.byref(full))
    sub = lambda **kw: tuple(kw.get(n, v) for n, v in zip(('h', 'env_of', 'm', 't', 'k', 'e', 'seed', 'seed_dev', 'w', 'ret', 'smooth', 'gain', 'out'), a))  # noqa: E731
    invalid = [(sub(h=None), b'engine'), (sub(out=None), b'out'), (sub(ret=None), b'null ret'), (sub(out=C.byref(one(weights=vp(bufs['weights'])))), b'null out->elites'),
               (sub(m=-1), b'n_states'), (sub(m=2 ** 27 + 1), b'n_states'), (sub(t=0), b'n_steps'), (sub(t=32768), b'n_steps'), (sub(k=0), b'n_samples'),
               (sub(k=65537), b'n_samples'), (sub(e=0), b'n_elites'), (sub(e=K + 1), b'n_elites'), (sub(m=65537, t=64, k=1024), b'above 2^32'),
               (sub(m=65536, t=65, k=1024), b'above 2^32'), (sub(smooth=65536), b'smooth'), (sub(gain=0), b'gain'), (sub(gain=65536), b'gain'),
               (sub(env_of=vp(eo, 2)), b'aligned'), (sub(ret=vp(ret, 2)), b'aligned'), (sub(w=vp(w, 1)), b'aligned'),
               (sub(out=C.byref(one(elites=vp(bufs['elites'], 2)))), b'aligned'), (sub(out=C.byref(one(elites=vp(bufs['elites']), elite_min=vp(bufs['elite_min'], 1)))), b'aligned'),
               (sub(out=C.byref(one(elites=vp(bufs['elites']), weights=vp(bufs['weights'], 1)))), b'aligned'),
               (sub(out=C.byref(one(elites=vp(ret, 4 * (K * N - 1))))), b'overlaps'), (sub(env_of=vp(eo), out=C.byref(one(elites=vp(eo, 4 * (N - 1))))), b'overlaps'),
               (sub(out=C.byref(one(elites=vp(bufs['elites']), elite_min=vp(bufs['elites'], 4 * (E * N - 1))))), b'overlaps'),
               (sub(out=C.byref(one(elites=vp(bufs['elites']), weights=vp(bufs['elites'], 4 * E * N - 2)))), b'overlaps'),
               (sub(w=vp(w), out=C.byref(one(elites=vp(bufs['elites']), weights=vp(w, 2)))), b'overlaps'),                        # shifted by one element: not in place
               (sub(w=vp(w, 2), out=C.byref(one(elites=vp(bufs['elites']), weights=vp(w)))), b'overlaps'),
               (sub(w=vp(w), out=C.byref(one(elites=vp(w, 12 * T * N - 4)))), b'overlaps')]
    for args, word in invalid:
        assert lib.cw_shoot_refit(*args, st) == L.CW_ERR_INVALID, word
        assert word in lib.cw_last_error(), (word, lib.cw_last_error())
    assert lib.cw_shoot_refit(*sub(out=C.byref(one(elites=vp(ret, 4 * K * N)))), st) == L.CW_OK      # (adjacent is not overlapping: the spare rows of ret)
    torch.cuda.synchronize()
    assert env.expand_skipped == 0
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 6. cem
def test_cem_is_the_hand_written_loop(engine70):
    """cem(iters=3) against shoot() + shoot_refit() written out, byte for byte in every field -- from uniform, from a caller's weights (left as they were)
    and with a seed word on the device"""
    env, T, K, E = engine70, 6, 20, 5
    names = ('best_ret', 'best_sample', 'best_action', 'length', 'done', 'achieved_mask', 'hdr', 'slot_pos', 'plan', 'ret')
    mine = _dev(_weights(T, N1, 3), np.uint16)
    kept = mine.clone()
    for seed, start in ((2 ** 64 - 2, None), (11, mine)):
        got = env.cem(T, K, E, 3, seed, weights=start, smooth=0, gain=2, fields=names)
        w = None if start is None else start.clone()
        for i in range(3):
            s = (seed + i) % 2 ** 64
            shot = env.shoot(T, K, s, weights=w, fields=names)
            fit = env.shoot_refit(shot['ret'], E, T, s, weights=w, smooth=0, gain=2)
            w = fit['weights']
        assert set(got) == set(names) | {'weights', 'elite_min'}
        for f in names:
            assert torch.equal(got[f], shot[f]), (seed, f)
        assert torch.equal(got['weights'].view(torch.int16), w.view(torch.int16)) and torch.equal(got['elite_min'], fit['elite_min'])
        assert (got['weights'].view(torch.int16) == 0).any()                      # smooth = 0: an action no elite drew is forbidden from then on
    assert torch.equal(mine.view(torch.int16), kept.view(torch.int16))            # a caller's tensor is never written
    word = torch.tensor([2 ** 63 + 5], dtype=torch.uint64, device='cuda')
    a, b = env.cem(T, K, E, 3, word, fields=names), env.cem(T, K, E, 3, 2 ** 63 + 5, fields=names)
    assert all(torch.equal(a[f].view(torch.uint8), b[f].view(torch.uint8)) for f in a)
    again = env.cem(T, K, E, 2, 2 ** 63 + 8, weights=b['weights'], fields=names, out=b)                  # the warm start: every buffer again, in place
    assert all(again[f] is b[f] for f in b) and not torch.equal(again['weights'].view(torch.int16), a['weights'].view(torch.int16))
    five = env.cem(T, K, E, 5, 2 ** 63 + 5, fields=names)                        # three iterations and two more are five
    assert all(torch.equal(again[f].view(torch.uint8), five[f].view(torch.uint8)) for f in five)


@pytest.mark.parametrize('T,K,E', [(6, 8, 3), (12, 33, 8)])
def test_cem_against_the_oracle(T, K, E):
    """two iterations on the 600-state recipe: shoot_check.expected_shoot (the oracle) and refit_check.expected_refit chained by hand"""
    seed, smooth, gain = 1, 1, 2
    dense, init_grids, first = recipe_shots(T, K, seed)
    M = len(dense['hold'])
    fit1 = rc.expected_refit(first['ret'], E, T, seed, None, smooth, gain)
    assert rc.split_ties(first['ret'], E).sum() >= 100
    second = expected_shoot(dense, init_grids, T, K, seed + 1, RECIPE_KW, fit1['weights'])
    fit2 = rc.expected_refit(second['ret'], E, T, seed + 1, fit1['weights'], smooth, gain)
    assert (second['best_ret'] != first['best_ret']).any()
    env, _, _ = make_env(M, *np_states(M, 900), obs_mode='state', auto_reset=False, **RECIPE_KW)
    env.reset()
    before = take(env)
    assert np.array_equal(before['state_init_grid'], init_grids)
    hdr, pos = encode(dense, menu=before['hdr'][:, 3])
    got = env.cem(T, K, E, 2, seed, _dev(hdr), _dev(pos.view(np.int16), np.int16), _dev(np.arange(M), np.int32), smooth=smooth, gain=gain,
                  fields=('best_ret', 'best_sample', 'best_action', 'length', 'done', 'plan', 'ret'))
    got = _np(got)
    for f in ('ret', 'best_ret', 'best_sample', 'best_action', 'length', 'plan'):
        assert np.array_equal(got[f], second[f]), f
    assert np.array_equal(got['done'].view(np.uint8), second['done'].astype(np.uint8))
    assert np.array_equal(got['weights'], fit2['weights']) and np.array_equal(got['elite_min'], fit2['elite_min'])
    one = _np(env.cem(T, K, E, 1, seed, _dev(hdr), _dev(pos.view(np.int16), np.int16), _dev(np.arange(M), np.int32), smooth=smooth, gain=gain, fields=('ret',)))
    assert np.array_equal(one['ret'], first['ret']) and np.array_equal(one['weights'], fit1['weights']) and np.array_equal(one['elite_min'], fit1['elite_min'])
    after = take(env)
    assert all(np.array_equal(before[k], after[k]) for k in before)
    env.close()


def test_cem_captured_into_a_graph_with_a_step():
    """torch.cuda.graph around step(actions) + cem(out=..., seed=tensor): the calls only enqueue; each replay steps the env and plans from the state it
    reaches with the seed the word then holds, equal to the eager calls with that seed on a twin engine in the same state"""
    N, T, K, E = 300, 6, 20, 5
    names = ('best_ret', 'best_sample', 'best_action', 'length', 'done', 'achieved_mask', 'hdr', 'slot_pos', 'plan', 'ret')
    env, keys, pos = make_env(N, *np_states(N, 93000), obs_mode='state', auto_reset=False, **K5)
    twin, _, _ = make_env(N, keys, pos, obs_mode='state', auto_reset=False, **K5)
    for e in (env, twin):
        e.reset()
        spread(e, 5, 6)
        _walk_goals(e, 3, 94)
    assert torch.equal(env.hdr, twin.hdr) and torch.equal(env.slot_pos, twin.slot_pos)
    acts = _dev(np.random.RandomState(95).randint(0, 6, N))
    word = torch.tensor([2 ** 64 - 3], dtype=torch.uint64, device='cuda')
    out = env.cem(T, K, E, 2, word, fields=names)                                 # (warm-up outside the capture: the buffers, the env's scratch)
    env.synchronize()
    for t in out.values():
        t.view(torch.uint8).fill_(0xA5)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.step_async(acts)
        assert env.cem(T, K, E, 2, word, fields=names, out=out) is not None
    assert all(bool((t.view(torch.uint8) == 0xA5).all()) for t in out.values())          # (capturing ran nothing)
    plans = []
    for rnd, value in enumerate((2 ** 64 - 3, 2 ** 64 - 1, 1)):                    # the word bumped between the replays, past the wrap
        acts.copy_(_dev(np.random.RandomState(96 + rnd).randint(0, 6, N)))
        word.copy_(torch.tensor([value], dtype=torch.uint64))
        g.replay()
        twin.step(acts)
        eager = twin.cem(T, K, E, 2, value, fields=names)
        for f in eager:
            assert torch.equal(out[f].view(torch.uint8), eager[f].view(torch.uint8)), (rnd, f)
        assert torch.equal(env.hdr, twin.hdr)
        plans.append(out['plan'].clone())
    assert not torch.equal(plans[0], plans[1]) and not torch.equal(plans[1], plans[2])
    torch.cuda.synchronize()
    env.close()
    twin.close()
