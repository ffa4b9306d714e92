"""GPU tier of the visited set: cw_seen_claim_kernel / cw_seen_resolve_kernel / cw_seen_clear_kernel through CraftingWorldVecEnv.seen_insert, seen_clear and
seen_reserve.  Every call is checked row by row with seen_check.check_seen_call (itself tested on the CPU, tests/test_seen_logic.py) against a Python set of
the keys: the rows that take part, the sentinel in those that do not, the set's counters, and -- where the engine is snapshotted -- the engine before and
after byte for byte.  With 64-bit tags and enough capacity the match is exact and both counters stay 0; in the overflow and collision tests rows may deviate
only as "fresh", and only as often as the counters grew.  No timing."""
import ctypes as C

import numpy as np
import pytest
import torch

from engines import ENGINES, K5, N1, k_of, n_cu
from masked_check import spread, take
from oracle_replay import make_env, np_states
from records_gpu import SENT, dev as _dev, walked_engine
from seen_check import SeenModel, check_seen_call, key_of

pytestmark = pytest.mark.gpu


def _sentinel_out(M, fields=('fresh', 'first')):
    out = {}
    if 'fresh' in fields:
        out['fresh'] = torch.full((M,), SENT, dtype=torch.uint8, device='cuda').view(torch.bool)
    if 'first' in fields:
        out['first'] = torch.full((M, 4), SENT, dtype=torch.uint8, device='cuda').view(torch.int32).squeeze(-1)
    return out


def _counters(env):
    return env._seen_ctl.cpu().numpy().copy()


def _insert(env, model, hdr, pos, group=None, *, exact=True, fields=('fresh', 'first'), engine=False):
    """seen_insert of numpy records into sentinel-filled buffers, checked against `model` (which then holds them) -> (outputs as numpy, deviating rows)"""
    M = len(hdr)
    out = _sentinel_out(M, fields)
    c0, before = _counters(env), take(env) if engine else None
    g = None if group is None else _dev(group, np.int32)
    r = env.seen_insert(_dev(hdr), _dev(pos.view(np.int16), np.int16), g, fields=fields, out=out)
    assert all(r[f] is out[f] for f in fields)
    got = {f: out[f].view(torch.uint8).cpu().numpy() if f == 'fresh' else out[f].cpu().numpy() for f in fields}
    n_off = check_seen_call(model, dict(hdr=hdr, slot_pos=pos, group=group, num_envs=env.num_envs), got, SENT, c0, _counters(env), before,
                            take(env) if engine else None, exact=exact)
    return got, n_off


def _random_records(n, seed):
    """n records of random bytes with distinct keys (a record is never an address: the set only packs, hashes and compares it)"""
    r = np.random.RandomState(seed)
    hdr, pos = r.randint(0, 256, (n, 16)).astype(np.uint8), r.randint(0, 65536, (n, 8)).astype(np.uint16)
    assert len(np.unique(key_of(hdr, pos, np.zeros(n)), axis=0)) == n
    return hdr, pos


@pytest.fixture(scope='module')
def engine70():
    env = walked_engine(97000, 6)
    yield env
    env.close()


@pytest.fixture()
def fresh_set(engine70):
    engine70.seen_reserve(1 << 16)
    assert engine70.seen_slots == 1 << 17 and (engine70.seen_size, engine70.seen_overflow, engine70.seen_collisions) == (0, 0, 0)
    return engine70, SeenModel()


# ------------------------------------------------------------------------------------------------------------------------------ 1. shapes
@pytest.mark.parametrize('M', [1, 63, 64, 65])
def test_small_batches(fresh_set, M):
    env, model = fresh_set
    hdr, pos = _random_records(40, M)
    pick = np.random.RandomState(M).randint(0, 40, M)
    group = np.random.RandomState(M + 1).randint(0, 3, M)
    got, _ = _insert(env, model, hdr[pick], pos[pick], group, engine=True)
    assert got['fresh'].sum() == len(model) == env.seen_size
    got, _ = _insert(env, model, hdr[pick], pos[pick], group)                       # the same call again: everything has been seen
    assert (got['first'] == -1).all() and not got['fresh'].any()


def test_no_rows(fresh_set):
    env, _ = fresh_set
    r = env.seen_insert(torch.empty((0, 16), dtype=torch.uint8, device='cuda'), torch.empty((0, 8), dtype=torch.int16, device='cuda'))
    assert tuple(r['fresh'].shape) == (0,) and r['fresh'].dtype == torch.bool and tuple(r['first'].shape) == (0,) and r['first'].dtype == torch.int32
    assert env.seen_size == 0


def test_the_successors_of_expand(fresh_set):
    """6 x 70 successors, the default group j % num_envs: an action that changes nothing brings its parent's key again"""
    env, model = fresh_set
    r = env.expand(fields=('hdr', 'slot_pos', 'changed'))
    hdr, pos = r['hdr'].reshape(-1, 16).cpu().numpy(), r['slot_pos'].reshape(-1, 8).cpu().numpy().view(np.uint16)
    got, _ = _insert(env, model, hdr, pos, None, engine=True)
    assert 70 <= got['fresh'].sum() < 6 * N1 and ((got['first'] >= 0) & (got['first'] != np.arange(6 * N1))).any()
    got, _ = _insert(env, model, env.hdr.cpu().numpy(), env.slot_pos.cpu().numpy().view(np.uint16), None)        # the parents: seen where some action changed nothing
    unchanged = ~r['changed'].cpu().numpy().all(axis=0)
    assert np.array_equal(got['first'] == -1, unchanged) and unchanged.any()          # (nearly every state has some action that does nothing)


def test_past_the_first_grid_stride_round(engine70):
    """one row more than the launch's lanes (8 workgroups of 256 per CU): the last row is a second-round row of lane 0; keys repeat within and across rounds"""
    env = engine70
    M = n_cu() * 8 * 256 + 1
    env.seen_reserve(1 << 16)
    hdr, pos = _random_records(5000, 7)
    pick = np.random.RandomState(8).randint(0, 5000, M)
    pick[-1] = pick[0]
    group = (np.arange(M) % 3).astype(np.int64)
    group[[5, M - 2]] = -1
    group[M - 1] = group[0]
    model = SeenModel()
    got, _ = _insert(env, model, hdr[pick], pos[pick], group)
    assert got['first'][M - 1] == 0 and got['fresh'][0] == 1
    assert env.seen_size == len(model) and 14000 < len(model) <= 15000


# ------------------------------------------------------------------------------------------------------------------------------ 2. contents
def test_copies_of_one_record(fresh_set):
    """4 096 copies: every row bids for one slot; only row 0 is fresh and first is 0 everywhere"""
    env, model = fresh_set
    hdr, pos = _random_records(1, 3)
    got, _ = _insert(env, model, np.repeat(hdr, 4096, axis=0), np.repeat(pos, 4096, axis=0), np.zeros(4096, np.int64))
    assert (got['first'] == 0).all() and got['fresh'][0] == 1 and got['fresh'].sum() == 1 and env.seen_size == 1


def test_distinct_rows_pairs_and_the_same_call_again(fresh_set):
    env, model = fresh_set
    hdr, pos = _random_records(3000, 4)
    zeros = np.zeros(3000, np.int64)
    got, _ = _insert(env, model, hdr[:1000], pos[:1000], zeros[:1000])
    assert got['fresh'].all() and np.array_equal(got['first'], np.arange(1000))
    order = np.random.RandomState(5).permutation(np.repeat(np.arange(1000, 3000), 2))          # each key twice, shuffled
    got, _ = _insert(env, model, hdr[order], pos[order], np.zeros(4000, np.int64))
    assert got['fresh'].sum() == 2000 and ((got['first'] >= 0) & (got['first'] < np.arange(4000))).sum() == 2000
    for fields in (('fresh', 'first'), ('first',), ('fresh',)):
        got, _ = _insert(env, model, hdr[order], pos[order], np.zeros(4000, np.int64), fields=fields)
        assert all((got[f] == (-1 if f == 'first' else 0)).all() for f in fields)
    assert env.seen_size == 3000


def test_negative_groups_and_groups_apart(fresh_set):
    env, model = fresh_set
    hdr, pos = _random_records(50, 6)
    pick = np.arange(400) % 50
    group = (np.arange(400) // 50).astype(np.int64)                                  # the same 50 records in 8 groups: apart
    group[::7] = -1 - (np.arange(400)[::7] % 5)
    group[399] = 2 ** 31 - 1
    got, _ = _insert(env, model, hdr[pick], pos[pick], group)
    part = group >= 0
    assert got['fresh'][part].all() and len(model) == part.sum()
    got, _ = _insert(env, model, hdr[:50], pos[:50], np.full(50, 8, np.int64))        # a ninth group: all new
    assert got['fresh'].all()
    got, _ = _insert(env, model, hdr[:50], pos[:50], np.full(50, 3, np.int64))        # the fourth again: seen, but for the rows that took no part then
    assert np.array_equal(got['first'] == -1, group[150:200] >= 0)


def test_what_merges_and_what_does_not(fresh_set):
    env, model = fresh_set
    hdr, pos = _random_records(64, 9)
    group = np.zeros(64, np.int64)
    _insert(env, model, hdr, pos, group)
    x = hdr.copy()
    x[:, 3] ^= 0xFF                                                                  # menu
    x[:, 8:10] = np.random.RandomState(1).randint(0, 256, (64, 2))                   # step_num
    x[:, 10] ^= 0xFD                                                                 # flag bit 0 and the low bits of the success count
    x[:, 11] ^= 0xFF
    got, _ = _insert(env, model, x, pos, group)
    assert (got['first'] == -1).all()
    for j, (byte, bit) in enumerate([(b, k) for b in (0, 1, 2, 4, 5, 6, 7, 12, 13, 14, 15) for k in (0, 7)] + [(10, 1)]):
        y = hdr.copy()
        y[:, byte] ^= 1 << bit
        got, _ = _insert(env, model, y, pos, group)
        assert got['fresh'].all(), (byte, bit)
    for slot in range(8):
        q = pos.copy()
        q[:, slot] ^= 1 << (2 * slot)
        got, _ = _insert(env, model, hdr, q, group)
        assert got['fresh'].all(), slot


# ------------------------------------------------------------------------------------------------------------------------------ 3. what equal keys promise
@pytest.mark.parametrize('S', [5, 21])
def test_equal_keys_have_equal_successors(S):
    """records that differ only in what the key leaves out: expand() gives equal reward, changed and achieved and successors with equal keys under every action;
    done differs only by the time-out.  21 x 21: slot cells above 255 survive the key."""
    env, _, _ = make_env(N1, *np_states(N1, 98000 + S), obs_mode='state', auto_reset=False, **k_of(S))
    env.reset()
    spread(env, 9, 5)
    hdr, pos = env.hdr.cpu().numpy(), env.slot_pos.cpu().numpy().view(np.uint16)
    if S == 21:
        assert (pos[pos < S * S] > 255).any()
    x = hdr.copy()
    x[:, 3] = np.arange(N1) % 7
    x[:, 8], x[:, 9] = np.arange(N1) % 5, 0
    x[:, 10] = (x[:, 10] & 2) | ((np.arange(N1) % 2)) | 4
    group = np.arange(N1)
    assert np.array_equal(key_of(x, pos, group), key_of(hdr, pos, group)) and (x != hdr).any(axis=1).all()
    a = env.expand(_dev(hdr), _dev(pos.view(np.int16), np.int16))
    b = env.expand(_dev(x), _dev(pos.view(np.int16), np.int16))
    for f in ('reward', 'changed', 'achieved_mask'):
        assert torch.equal(a[f], b[f]), f
    assert a['changed'].any() and not a['changed'].all()
    g6 = np.tile(group, 6)
    ka = key_of(a['hdr'].reshape(-1, 16).cpu().numpy(), a['slot_pos'].reshape(-1, 8).cpu().numpy(), g6)
    kb = key_of(b['hdr'].reshape(-1, 16).cpu().numpy(), b['slot_pos'].reshape(-1, 8).cpu().numpy(), g6)
    assert np.array_equal(ka, kb)
    env.seen_reserve(4096)                                                           # ... and the set agrees: the twins' successors have all been seen
    model = SeenModel()
    _insert(env, model, a['hdr'].reshape(-1, 16).cpu().numpy(), a['slot_pos'].reshape(-1, 8).cpu().numpy().view(np.uint16), None)
    got, _ = _insert(env, model, b['hdr'].reshape(-1, 16).cpu().numpy(), b['slot_pos'].reshape(-1, 8).cpu().numpy().view(np.uint16), None)
    assert (got['first'] == -1).all()
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 4. overflow and collisions
def test_overflow_is_counted_and_errs_on_the_safe_side(engine70):
    env = engine70
    env.seen_reserve(16)
    assert env.seen_slots == 32
    hdr, pos = _random_records(1000, 10)
    model, group = SeenModel(), np.zeros(1000, np.int64)
    got, _ = _insert(env, model, hdr, pos, group, exact=False)
    assert got['fresh'].all()                                                        # (all distinct: fresh is also what the model says)
    assert env.seen_overflow >= 1000 - 32 and env.seen_size <= env.seen_slots == 32 and env.seen_size + env.seen_overflow + env.seen_collisions == 1000
    got, n_off = _insert(env, model, hdr, pos, group, exact=False)                    # again: the keys held are seen, the others overflow again -- fresh, and counted
    assert n_off == 1000 - env.seen_size and (got['first'] == -1).sum() == env.seen_size
    assert env.seen_overflow + env.seen_collisions >= 2 * (1000 - 32)


def test_collisions_are_counted_and_full_tags_are_exact_again(engine70):
    env = engine70
    env.seen_reserve(1024, tag_bits=4)                                                # (half full at the end: a row's probes meet other keys' slots, one in 15 under its tag)
    hdr, pos = _random_records(1000, 11)
    order = np.random.RandomState(12).permutation(np.repeat(np.arange(1000), 2))
    model, group = SeenModel(), np.zeros(2000, np.int64)
    got, n_off = _insert(env, model, hdr[order], pos[order], group, exact=False)
    assert env.seen_collisions > 0 and n_off > 0 and env.seen_size < 1000
    assert env.seen_size + env.seen_overflow + env.seen_collisions >= 1000            # (a key is held, or both its rows were turned away)
    env.seen_clear()
    assert (env.seen_size, env.seen_overflow, env.seen_collisions) == (0, 0, 0)
    env.seen_reserve(1024)                                                            # full tags: the same rows, exact
    model = SeenModel()
    got, _ = _insert(env, model, hdr[order], pos[order], group)
    assert got['fresh'].sum() == 1000 == env.seen_size


def test_the_last_usable_epoch_and_the_spent_one(engine70):
    """The epoch is word 3 (CW_SEEN_EPOCH) of the control block cw_seen_counters names; the test writes it through a view of its own.  At the LAST USABLE
    epoch, CWH_SEEN_MAX_EPOCH, a bid epoch << 28 | row fills the owner word up to bit 63: 300 new records (40 of them a second time, further down: first is
    the smaller row) mixed with 300 held ones are exact against the model, and the epoch moves on to MAX_EPOCH + 1.  That epoch is SPENT: the same rows again
    are all reported fresh with first = row and counted as overflow, row for row; the rows of a negative group keep the sentinel; keys held, collisions and
    the epoch itself do not move -- a deviation in the safe direction, which check_seen_call(exact=False) accepts.  seen_clear() makes the set exact again."""
    from gym_craftingworld_amd import _lib as L
    from gym_craftingworld_amd._wrap import tensor_view
    env = engine70
    env.seen_reserve(4096)
    p = C.c_void_p()
    assert env._lib.cw_seen_counters(env._h, C.byref(p)) == L.CW_OK
    ctl = tensor_view(p.value, (5,), torch.int64, env.device.index)                   # size, overflow, collisions, EPOCH, ticket
    epoch = lambda: int(ctl[3].item())  # noqa: E731
    hdr, pos = _random_records(600, 14)
    model = SeenModel()
    _insert(env, model, hdr[:300], pos[:300], np.zeros(300, np.int64))
    assert epoch() == 1 and env.seen_size == 300
    ctl[3] = L.CWH_SEEN_MAX_EPOCH
    torch.cuda.synchronize()
    rows = np.concatenate([np.random.RandomState(15).permutation(600), 300 + np.arange(40) * 7])      # 600 records, and 40 of the new ones again
    group = np.zeros(640, np.int64)
    group[[7, 311, 599, 639]] = [-1, -4, -1, -2]
    part = group >= 0
    got, _ = _insert(env, model, hdr[rows], pos[rows], group, engine=True)
    want, met = np.full(640, -1, np.int64), {}
    for j in np.flatnonzero(part & (rows >= 300)):                                   # a new record: the smallest participating row that brings it
        want[j] = met.setdefault(int(rows[j]), int(j))
    assert np.array_equal(got['first'][part], want[part]) and (got['first'][part] == -1).sum() >= 290
    assert ((want[600:] >= 0) & (want[600:] < 600)).sum() >= 35
    assert epoch() == L.CWH_SEEN_MAX_EPOCH + 1 and env.seen_size == len(model)
    c0 = _counters(env)
    got, n_off = _insert(env, model, hdr[rows], pos[rows], group, exact=False, engine=True)           # spent: the set neither looks nor learns
    assert np.array_equal(got['first'][part], np.flatnonzero(part)) and (got['fresh'][part] == 1).all()
    assert (got['fresh'][~part] == SENT).all() and (got['first'].view(np.uint8).reshape(-1, 4)[~part] == SENT).all()
    assert (_counters(env) - c0).tolist() == [0, int(part.sum()), 0] and n_off == part.sum() and epoch() == L.CWH_SEEN_MAX_EPOCH + 1
    assert int(ctl[4].item()) == 0                                                    # (the ticket is back at 0 for the next call)
    env.seen_clear()
    assert epoch() == 0 and _counters(env).tolist() == [0, 0, 0]
    model = SeenModel()
    got, _ = _insert(env, model, hdr[rows], pos[rows], group)
    assert got['fresh'][part].sum() == len(model) == env.seen_size and epoch() == 1


# ------------------------------------------------------------------------------------------------------------------------------ 5. call order, engines, capture
def test_clear_and_reserve_drop_the_keys(fresh_set):
    env, model = fresh_set
    hdr, pos = _random_records(300, 13)
    group = np.zeros(300, np.int64)
    _insert(env, model, hdr, pos, group)
    env.seen_clear()
    assert env.seen_size == 0
    got, _ = _insert(env, SeenModel(), hdr, pos, group)
    assert got['fresh'].all()
    env.seen_reserve(1 << 10)
    assert env.seen_slots == 1 << 11 and env.seen_size == 0
    got, _ = _insert(env, SeenModel(), hdr, pos, group)
    assert got['fresh'].all() and env.seen_size == 300
    env.seen_reserve(0)
    assert env.seen_slots == 0 and env.seen_size == 0


def test_call_order_and_bad_arguments():
    from gym_craftingworld_amd import CraftingWorldVecEnv, _lib as L
    env = CraftingWorldVecEnv(8, obs_mode='state', auto_reset=False, seed=3, **K5)
    lib, h, st = env._lib, env._h, env._stream()
    vp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    hdr, pos = torch.zeros((8, 16), dtype=torch.uint8, device='cuda'), torch.zeros((8, 8), dtype=torch.int16, device='cuda')
    out = _sentinel_out(8)
    full = L.cw_seen_out(fresh=out['fresh'].data_ptr(), first=out['first'].data_ptr())
    env.seen_reserve(64)
    assert lib.cw_seen_insert(h, None, vp(hdr), vp(pos), 8, C.byref(full), st) == L.CW_ERR_STATE and b'before cw_reset' in lib.cw_last_error()
    assert lib.cw_seen_clear(h, st) == L.CW_ERR_STATE
    env.seen_reserve(0)
    env.reset()
    assert lib.cw_seen_insert(h, None, vp(hdr), vp(pos), 8, C.byref(full), st) == L.CW_ERR_STATE and b'no set reserved' in lib.cw_last_error()
    assert lib.cw_seen_clear(h, st) == L.CW_ERR_STATE and b'no set reserved' in lib.cw_last_error()
    p = C.c_void_p(1)
    assert lib.cw_seen_counters(h, C.byref(p)) == L.CW_ERR_STATE and not p.value and lib.cw_seen_slots(h) == 0
    with pytest.raises(L.CraftingWorldError):
        env.seen_insert(hdr, pos)
    with pytest.raises(L.CraftingWorldError):
        env.seen_clear()
    for bad in ((-1, 0), (2 ** 28 + 1, 0), (16, -1), (16, 64)):
        assert lib.cw_seen_reserve(h, *bad) == L.CW_ERR_INVALID
        with pytest.raises(ValueError):
            env.seen_reserve(bad[0], tag_bits=bad[1])
    env.seen_reserve(64, tag_bits=63)
    grp = torch.zeros(8, dtype=torch.int32, device='cuda')
    assert lib.cw_seen_insert(h, vp(grp), vp(hdr), vp(pos), 0, C.byref(full), st) == L.CW_OK                       # no rows: nothing enqueued
    torch.cuda.synchronize()
    assert all(bool((t.view(torch.uint8) == SENT).all()) for t in out.values())
    invalid = [((None, None, vp(hdr), vp(pos), 8, C.byref(full)), b'engine'), ((h, None, vp(hdr), vp(pos), 8, None), b'out'),
               ((h, None, None, vp(pos), 8, C.byref(full)), b'null hdr'), ((h, None, vp(hdr), None, 8, C.byref(full)), b'null slot_pos'),
               ((h, None, vp(hdr), vp(pos), 8, C.byref(L.cw_seen_out())), b'every field'),
               ((h, None, vp(hdr), vp(pos), -1, C.byref(full)), b'n_states'), ((h, None, vp(hdr), vp(pos), 2 ** 27 + 1, C.byref(full)), b'n_states'),
               ((h, None, vp(hdr, 8), vp(pos), 7, C.byref(full)), b'aligned'), ((h, None, vp(hdr), vp(pos, 2), 7, C.byref(full)), b'aligned'),
               ((h, vp(grp, 2), vp(hdr), vp(pos), 7, C.byref(full)), b'aligned'),
               ((h, None, vp(hdr), vp(pos), 7, C.byref(L.cw_seen_out(first=out['first'].data_ptr() + 2))), b'aligned'),
               ((h, None, vp(hdr), vp(pos), 8, C.byref(L.cw_seen_out(fresh=hdr.data_ptr() + 127))), b'overlaps'),
               ((h, None, vp(hdr), vp(pos), 8, C.byref(L.cw_seen_out(first=pos.data_ptr()))), b'overlaps'),
               ((h, vp(grp), vp(hdr), vp(pos), 8, C.byref(L.cw_seen_out(first=grp.data_ptr()))), b'overlaps'),
               ((h, None, vp(hdr), vp(pos), 8, C.byref(L.cw_seen_out(fresh=out['first'].data_ptr() + 31, first=out['first'].data_ptr()))), b'overlaps')]
    for args, word in invalid:
        assert lib.cw_seen_insert(*args, st) == L.CW_ERR_INVALID, word
        assert word in lib.cw_last_error(), (word, lib.cw_last_error())
    for bad in (dict(group=torch.zeros(7, dtype=torch.int32, device='cuda')), dict(group=np.zeros(8)), dict(group=[2 ** 31] * 8), dict(fields=[]),
                dict(fields=['fresh', 'seen']), dict(out={'fresh': out['fresh']}), dict(out=dict(out, first=out['first'].to(torch.int64)))):
        with pytest.raises(ValueError):
            env.seen_insert(hdr, pos, **bad)
    with pytest.raises(ValueError):
        env.seen_insert(None, None)
    torch.cuda.synchronize()
    assert env.seen_size == 0
    r = env.seen_insert(hdr.cpu().numpy(), pos.cpu().numpy(), [0, 0, 1, -1, 1, 2, -5, 0])          # the host-validated path
    assert r['first'].cpu().numpy()[[0, 1, 2, 4, 5, 7]].tolist() == [0, 0, 2, 2, 5, 0] and env.seen_size == 3
    env.close()


@pytest.mark.parametrize('engine', list(ENGINES))
def test_on_every_engine(engine):
    """the set of an engine of every kind, filled with the successors of its own states; the engine itself -- states, streams, buffers, frames, counters --
    byte for byte unchanged"""
    env, _, _ = make_env(N1, *np_states(N1, 99000), **ENGINES[engine], **K5)
    env.reset()
    spread(env, 7, 4)
    env.seen_reserve(1024)
    r = env.expand(fields=('hdr', 'slot_pos'))
    hdr, pos = r['hdr'].reshape(-1, 16).cpu().numpy(), r['slot_pos'].reshape(-1, 8).cpu().numpy().view(np.uint16)
    model = SeenModel()
    got, _ = _insert(env, model, hdr, pos, None, engine=True)
    assert got['fresh'].sum() == len(model) == env.seen_size
    group = np.arange(6 * N1) % 2 - (np.arange(6 * N1) % 5 == 0) * 9
    _insert(env, model, hdr, pos, group, engine=True)
    env.close()


def test_captured_into_a_graph_with_expand():
    """torch.cuda.graph around expand(out=...) + seen_insert(out=...): the calls only enqueue; the first replay equals the eager call on an empty set, the
    second finds every key seen -- the epoch advances on the device"""
    N = 300
    env, _, _ = make_env(N, *np_states(N, 93000), obs_mode='state', auto_reset=False, **K5)
    env.reset()
    spread(env, 5, 6)
    env.seen_reserve(4096)
    succ = env.expand(fields=('hdr', 'slot_pos'))
    out = _sentinel_out(6 * N)
    env.seen_insert(succ['hdr'], succ['slot_pos'], out=_sentinel_out(6 * N))          # (warm-up outside the capture)
    env.seen_clear()
    env.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.expand(fields=('hdr', 'slot_pos'), out=succ)
        env.seen_insert(succ['hdr'], succ['slot_pos'], out=out)
    assert all(bool((t.view(torch.uint8) == SENT).all()) for t in out.values()) and env.seen_size == 0       # (capturing ran nothing)
    g.replay()
    torch.cuda.synchronize()
    hdr, pos = succ['hdr'].reshape(-1, 16).cpu().numpy(), succ['slot_pos'].reshape(-1, 8).cpu().numpy().view(np.uint16)
    model = SeenModel()
    got = dict(fresh=out['fresh'].view(torch.uint8).cpu().numpy(), first=out['first'].cpu().numpy())
    c1 = _counters(env)
    check_seen_call(model, dict(hdr=hdr, slot_pos=pos, group=None, num_envs=N), got, SENT, np.zeros(3, np.int64), c1, None, None, exact=True)
    assert N <= got['fresh'].sum() == len(model) < 6 * N
    g.replay()
    torch.cuda.synchronize()
    assert bool((out['first'] == -1).all()) and not bool(out['fresh'].any()) and np.array_equal(_counters(env), c1)
    g.replay()
    torch.cuda.synchronize()
    assert bool((out['first'] == -1).all())
    env.close()
