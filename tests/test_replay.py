"""GPU tier: the replay buffer of packed records against tests/replay_check.py's model, bit for bit.  Every push is checked against two independent
witnesses -- expand()'s row for the action taken, and what the following step() returns -- and against the model's episode rule; every sample against the
model's rows, sentinel-filled outputs included; the tests assert their own coverage from the model.  Purity, the frames of a sample end to end, graph
capture and the entry points' errors."""
import ctypes as C

import numpy as np
import pytest
import torch

import replay_check as rc
from engines import ENGINES, K5, N1
from masked_check import spread, take
from oracle_replay import make_env, np_states
from records_gpu import dev, walk_goals

pytestmark = pytest.mark.gpu

MAX_STEPS = K5['max_steps']
SENT = 0xA5
LS, BS, HERS = (1, 2, 3, 8), (1, 63, 64, 65, 257, 1000), (0, 1, 32768, 65536)
ACTION_DTYPES = (np.uint8, np.int32, np.int64)
OUT_OF_RANGE = {np.uint8: (6, 255, 128), np.int32: (-1, 6, 2 ** 31 - 1), np.int64: (2 ** 32 + 2, -1, -2 ** 40)}


def engine(n, seed, **kw):
    env, _, _ = make_env(n, *np_states(n, seed), **dict(K5, **kw))
    env.reset()
    return env


def view(env):
    torch.cuda.synchronize()
    return {f: t.cpu().numpy() for f, t in env.replay_view().items()}


def a_model(env, L):
    return rc.ReplayModel(L, env.num_envs, env.MAX_STEPS, (1 << len(env.task_list)) - 1)


def actions_of(n, k, rng):
    """the actions of push k: the dtype cycles through cw_step's three, and a few envs get ids outside 0..5"""
    dt = ACTION_DTYPES[k % 3]
    a = rng.randint(0, 6, n).astype(dt)
    for j, bad in enumerate(OUT_OF_RANGE[dt]):
        if n > 3 * j + 2:
            a[(3 * j + 2 + k) % n] = bad
        elif n == 1 and k % 2 and j == k // 2 % 3:                                # (a single env: every other push)
            a[0] = bad
    return a


def witness(env, actions):
    """the transition every env is about to make, from expand() and the public state -> ReplayModel.push's arguments without the goal record"""
    hdr, pos = env.hdr.cpu().numpy().copy(), env.slot_pos.cpu().numpy().copy()
    ex = {f: (t.view(torch.uint8) if t.dtype is torch.bool else t).cpu().numpy() for f, t in env.expand().items()}
    a = np.asarray(actions).astype(np.int64)
    valid = (a >= 0) & (a <= 5)
    # an id outside 0..5 is the state-preserving step: that is the row of a pickup or a drop that fails -- one of the two always does (a pickup needs
    # an empty hand, a drop a full one), and a failed one changes nothing but step_num and flag bit 0
    idle = np.where(ex['changed'][4] == 0, 4, 5)
    assert (ex['changed'][idle, np.arange(len(a))] == 0).all()
    row = np.where(valid, a, idle)
    j = np.arange(len(a))
    return dict(hdr=hdr, slot_pos=pos, next_hdr=ex['hdr'][row, j], next_slot_pos=ex['slot_pos'][row, j], action=a, reward=ex['reward'][row, j],
                done=ex['done'][row, j], changed=np.where(valid, ex['changed'][row, j], 0))


def push(env, model, actions, step=True):
    """replay_push(actions) checked against the model fed by the witnesses, then (step=True) step(actions) checked against the stored transition"""
    t = witness(env, actions)
    goal_oh = env.one_hot(which='goal')
    a_dev = actions if env.host_outputs else dev(actions, actions.dtype)
    env.replay_push(a_dev)
    v = view(env)
    slot = model.n % model.L
    gh, gp = v['goal_hdr'][slot], v['goal_slot_pos'][slot]
    want12 = np.zeros((env.num_envs, 12), np.uint8)                               # THE GOAL RECORD: hold 0, the menu id, achieved = desired = the env's mask,
    want12[:, 3], want12[:, 4:6], want12[:, 6:8] = t['hdr'][:, 3], t['hdr'][:, 6:8], t['hdr'][:, 6:8]      # step_num and flags 0
    want12[:, 0:2] = gh[:, 0:2]
    assert np.array_equal(gh[:, :12], want12)
    assert torch.equal(env.one_hot_states(dev(gh), dev(gp, np.int16)), goal_oh)   # ... agent cell, codes and positions: the goal state itself
    rc.check_push(model, dict(t, goal_hdr=gh, goal_slot_pos=gp), v)
    if step:
        env.step(a_dev)
        torch.cuda.synchronize()
        assert np.array_equal(env.reward.cpu().numpy(), t['reward']) and np.array_equal(env.done.cpu().numpy(), t['done'].astype(bool))
        assert np.array_equal(env.achieved_mask.cpu().numpy().view(np.uint16), rc.u16(t['next_hdr'], 4))
        if not env.auto_reset:
            assert np.array_equal(env.hdr.cpu().numpy(), t['next_hdr']) and np.array_equal(env.slot_pos.cpu().numpy(), t['next_slot_pos'])
    return t


def device_sentinels(B):
    out = {}
    for f, a in rc.sentinels(B, SENT).items():
        t = torch.as_tensor(a.view(np.int16) if a.dtype == np.uint16 else a, device='cuda')
        out[f] = t.view(torch.bool) if f == 'done' else t
    return out


def sample(env, model, B, seed, her, strategy, fields=rc.FIELDS):
    """replay_sample checked against the model -> the model's rows"""
    bufs = device_sentinels(B)
    before = {f: t.view(torch.uint8).cpu().numpy().view(rc.OUT_DTYPES[f]).reshape(t.shape) for f, t in bufs.items()}
    out = {f: bufs[f] for f in fields}
    assert env.replay_sample(B, seed, her=her / 65536, strategy=('future', 'final')[strategy], fields=fields, out=out) is out
    torch.cuda.synchronize()
    after = {f: t.view(torch.uint8).cpu().numpy().view(rc.OUT_DTYPES[f]).reshape(t.shape) for f, t in bufs.items()}
    return rc.check_sample(model, B, seed, her, strategy, before, after, fields)


# ------------------------------------------------------------------------------------------------------------------------------ 1. push: two witnesses, purity
def checkpoint(env):
    from gym_craftingworld_amd import _lib as L
    n = int(env._lib.cw_checkpoint_bytes(env._h))
    buf = np.empty(n, dtype=np.uint8)
    env._settle()
    L.check(env._lib.cw_checkpoint_save(env._h, buf.ctypes.data_as(C.c_void_p), n), 'cw_checkpoint_save', env._lib)
    return buf


def push_sequence(env, L, pushes, seed, pure_at=(0, 2)):
    """`pushes` rounds of push + step on `env`, each checked (push()); at the rounds `pure_at` the push is bracketed by take() and the checkpoint blob"""
    rng = np.random.RandomState(seed)
    env.replay_reserve(L)
    assert env.replay_bytes() > 106 * L * env.num_envs and env.replay_size() == 0
    model = a_model(env, L)
    rc.check_buffer(model, view(env))                                             # a new buffer is zero-filled and cleared
    seen_invalid = seen_done = 0
    for k in range(pushes):
        a = actions_of(env.num_envs, k, rng)
        if k in pure_at:
            before, blob = take(env), checkpoint(env)
            t = push(env, model, a, step=False)
            after = take(env)
            assert all(np.array_equal(before[f], after[f]) for f in before), [f for f in before if not np.array_equal(before[f], after[f])]
            assert np.array_equal(blob, checkpoint(env))                          # PURE: every buffer, stream, frame and counter, counters[3] included
            env.step(a if env.host_outputs else dev(a, a.dtype))
        else:
            t = push(env, model, a)
        seen_invalid += int((model.buf['action'][(model.n - 1) % L] == 255).sum())
        seen_done += int(t['done'].sum())
    assert env.replay_size() == pushes == model.n
    return model, seen_invalid, seen_done


@pytest.mark.parametrize('kind', list(ENGINES))
def test_push_against_expand_and_the_following_step(kind):
    env = engine(N1, 97000, **ENGINES[kind])
    spread(env, 11, 5)                                                            # into the episodes: time-outs within the pushes below
    model, invalid, done = push_sequence(env, 4, 11, 1)
    assert invalid >= 11 and done > 0
    assert int(env.counters[3].item()) == invalid                                 # the steps counted them; the pushes counted nothing
    env.replay_reserve(0)
    assert env.replay_bytes() == 0 and env.replay_size() == 0
    env.close()


def test_push_on_a_host_outputs_engine_with_host_actions():
    from gym_craftingworld_amd import CraftingWorldVecEnv
    env = CraftingWorldVecEnv(1, obs_mode='pixels_dirty', host_outputs=True, auto_reset=False, seed=5, **K5)
    env.reset()
    model, invalid, _ = push_sequence(env, 3, 8, 2, pure_at=(1,))
    assert model.n == 8 and invalid >= 1
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 2. the episode rule
def test_the_episode_rule_across_resets_loads_and_restores():
    """auto-resets, reset_envs, load_records, snapshot_load and imagine_obs(commit=True) between two pushes: the model's episode numbers, which follow from
    the pushed bytes alone, equal the buffer's (push() compares them), and every event is seen to cut the episodes it touched"""
    env = engine(N1, 97100, **ENGINES['dirty_ray_auto'])
    spread(env, 9, 6)
    env.snapshot_reserve(N1)
    L, rng = 8, np.random.RandomState(3)
    env.replay_reserve(L)
    model = a_model(env, L)
    cut = lambda before: model.env_episode.astype(np.int64) - before  # noqa: E731
    push(env, model, actions_of(N1, 0, rng))
    env.snapshot_save(np.arange(N1))
    saved = env.hdr.clone(), env.slot_pos.clone()
    t = push(env, model, actions_of(N1, 1, rng))
    ep = model.env_episode.astype(np.int64)
    env.reset_envs(indices=[3, 5, 64])
    push(env, model, actions_of(N1, 2, rng))
    assert (cut(ep)[[3, 5, 64]] == 1).all() and np.array_equal(cut(ep) == 1, t['done'].astype(bool) | np.isin(np.arange(N1), [3, 5, 64]))
    ep = model.env_episode.astype(np.int64)
    env.load_records(saved[0], saved[1], envs=[1, 2, 69], src=[1, 2, 69])         # back to where they were two pushes ago
    push(env, model, actions_of(N1, 3, rng))
    assert (cut(ep)[[1, 2, 69]] == 1).all() and (cut(ep) <= 1).all() and (cut(ep) == 1).sum() >= 3
    ep = model.env_episode.astype(np.int64)
    env.snapshot_load(envs=[7, 8], rows=[7, 8])
    push(env, model, actions_of(N1, 4, rng))
    assert (cut(ep)[[7, 8]] == 1).all()
    ep = model.env_episode.astype(np.int64)
    before = env.hdr.cpu().numpy().copy()
    env.imagine_obs(indices=[10, 11, 12, 13], desired=np.full(N1, 0x21, np.uint16), commit=True)
    moved = (env.hdr.cpu().numpy() != before).any(axis=1)
    push(env, model, actions_of(N1, 5, rng))
    assert moved[10:14].any() and (cut(ep)[10:14][moved[10:14]] == 1).all()       # a new goal is new bytes: a new episode
    auto_cuts = 0
    for k in range(6, 2 * L + 3):                                                 # and on through two wraps, auto-resets cutting as they come
        ep, was_done = model.env_episode.astype(np.int64), (model.buf['flags'][(model.n - 1) % L] & rc.DONE) != 0
        push(env, model, actions_of(N1, k, rng))
        assert np.array_equal(cut(ep) == 1, was_done)
        auto_cuts += int(was_done.sum())
    # 9 + 19 steps under max_steps 17: every env has timed out at least once, and the envs of the events above were cut a second time
    assert auto_cuts > 0 and model.env_episode.min() >= 1 and model.env_episode.max() >= 2
    env.close()


def test_a_finished_env_stepped_on_yields_episodes_of_length_one():
    env = engine(N1, 97200, **ENGINES['state_manual'])
    spread(env, 13, 7)
    L = 8
    env.replay_reserve(L)
    model, rng = a_model(env, L), np.random.RandomState(4)
    for k in range(MAX_STEPS + 3):                                                # no reset_envs: every env reaches max_steps and stays done
        push(env, model, actions_of(N1, k, rng))
    flags, ep = model.buf['flags'], model.buf['episode'].astype(np.int64)
    order = [(model.n - L + j) % L for j in range(L)]                             # the slots in position order
    done = (flags[order] & rc.DONE) != 0
    assert done[-4:].all()                                                        # more than max_steps steps: every env is past its time-out
    assert np.array_equal(np.diff(ep[order], axis=0), done[:-1].astype(np.int64))   # after a done transition the next one is an episode of its own
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 3. sample
def fill(env, model, pushes, seed):
    """pushes of a walked manual engine: done envs are reset as spread() resets them, and every push a few others too (discontinuities)"""
    rng = np.random.RandomState(seed)
    for k in range(pushes):
        push(env, model, actions_of(env.num_envs, k, rng))
        env.reset_envs(env.done)
        extra = [i for i in range(env.num_envs) if (i + k) % 7 == 3]
        if extra:
            env.reset_envs(indices=extra)
        if k % 3 == 1:
            walk_goals(env, 2, seed + k, every=3)                                 # goals within reach again after the resets


COVERAGE = ('future_later', 'reward_max', 'miss_changed', 'miss_unchanged', 'cut_by_done', 'cut_by_break', 'crosses_wrap', 'ends_newest')


@pytest.mark.parametrize('n', [1, 63, 64, 65, 70])
def test_sample_against_the_model(n):
    env = engine(n, 98000 + n, obs_mode='state', auto_reset=False)
    spread(env, 9, 3)
    walk_goals(env, 2, n)
    total = dict.fromkeys(COVERAGE + ('relabelled', 'plain'), 0)
    case = 0
    for L in LS:
        env.replay_reserve(L)
        model = a_model(env, L)
        assert sample(env, model, 5, 1, 65536, 0) is None                         # an empty buffer: no row is written
        fill(env, model, 2 * L + 3, 10 * n + L)                                   # the ring wraps twice
        for B in BS:
            for her in HERS:
                for strategy in (0, 1):
                    case += 1
                    fields = rc.FIELDS if case % 4 else ('hdr', 'goal_hdr', 'reward', 'done', 'future')      # (fields not handed over keep their sentinels)
                    rows = sample(env, model, B, 2 ** 64 - 7 * case, her, strategy, fields)
                    cov = model.coverage(rows)
                    assert cov['relabelled'] == (0 if her == 0 else B if her == 65536 else cov['relabelled'])
                    for key in total:
                        total[key] += cov[key]
        word = torch.tensor([2 ** 64 - 5], dtype=torch.uint64, device='cuda')
        sample(env, model, 65, 2 ** 64 - 2, 40000, 0)
        a = env.replay_sample(65, (9, word), her=0.6)
        b = env.replay_sample(65, 4, her=0.6)                                     # seed + *seed_dev mod 2^64
        assert all(torch.equal(a[f].view(torch.uint8), b[f].view(torch.uint8)) for f in a)
    if n > 1:
        assert all(total[key] > 0 for key in total), total                        # the test's own coverage, from the model alone
    env.close()


def test_sample_on_21x21():
    env = engine(64, 98500, obs_mode='state', auto_reset=False, size=(21, 21))
    spread(env, 5, 3)
    env.replay_reserve(3)
    model = a_model(env, 3)
    fill(env, model, 7, 6)
    for her, strategy in ((0, 0), (65536, 0), (32768, 1)):
        sample(env, model, 257, 77, her, strategy)
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 4. frames end to end
@pytest.mark.parametrize('kw', [dict(obs_mode='pixels_dirty', raster='ray'), dict(obs_mode='pixels', raster='alt')], ids=['dirty_ray', 'alt'])
def test_the_frames_of_a_sample(kw):
    n, L = 6, 8
    env = engine(n, 99000, keep_terminal_obs=True, **kw)
    spread(env, 12, 9)                                                            # episodes end within the pushes below
    env.replay_reserve(L)
    model, rng = a_model(env, L), np.random.RandomState(8)
    obs_at, goal_at, next_at, goal_oh = [], [], [], []
    for k in range(L):
        o = env._observation()
        obs_at.append(o['observation'].clone())
        goal_at.append(o['desired_goal'].clone())
        goal_oh.append(env.one_hot(which='goal').clone())
        a = rng.randint(0, 6, n).astype(np.uint8)
        push(env, model, a, step=False)
        o, _, done, info = env.step(dev(a))
        next_at.append(torch.where(done[:, None, None, None], info['terminal_observation'], o['observation']).clone())
    assert (model.buf['flags'] & rc.DONE).any()
    for her in (0, 65536):
        r = env.replay_sample(64, 3, her=her / 65536)
        torch.cuda.synchronize()
        i, p = r['env'].long(), r['slot'].long()                                  # n <= L: position = slot
        assert torch.equal(env.render_records(r['hdr'], r['slot_pos']), torch.stack(obs_at)[p, i])
        assert torch.equal(env.render_records(r['next_hdr'], r['next_slot_pos']), torch.stack(next_at)[p, i])
        goal = env.render_records(r['goal_hdr'], r['goal_slot_pos'])
        if her == 0:
            assert torch.equal(goal, torch.stack(goal_at)[p, i])
            assert torch.equal(env.one_hot_states(r['goal_hdr'], r['goal_slot_pos']), torch.stack(goal_oh)[p, i])
        else:                                                                     # relabelled: the achieved-goal image is the frame after step f
            assert torch.equal(goal, torch.stack(next_at)[r['future'].long(), i])
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 5. graph capture
def test_push_and_step_captured_into_a_graph():
    n, L = 64, 4
    env = engine(n, 99100, obs_mode='state', auto_reset=False)
    spread(env, 4, 2)
    env.replay_reserve(L)
    model, rng = a_model(env, L), np.random.RandomState(12)
    acts = dev(rng.randint(0, 6, n))
    push(env, model, acts.cpu().numpy())                                          # (warm-up outside the capture)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.replay_push(acts)
        env.step_async(acts)
    torch.cuda.synchronize()
    assert env.replay_size() == 1                                                 # capturing ran nothing
    for rnd in range(5):
        a = rng.randint(0, 6, n).astype(np.uint8)
        acts.copy_(dev(a))
        torch.cuda.synchronize()
        t = witness(env, a)
        slot = model.n % L
        g.replay()
        v = view(env)
        rc.check_push(model, dict(t, goal_hdr=v['goal_hdr'][slot], goal_slot_pos=v['goal_slot_pos'][slot]), v)
        assert np.array_equal(env.hdr.cpu().numpy(), t['next_hdr'])
    assert env.replay_size() == 6 and int(env.replay_view()['n'].item()) == 6    # n advanced on the device, replay after replay
    word = torch.tensor([100], dtype=torch.uint64, device='cuda')
    out = env.replay_sample(65, word, her=0.5)
    torch.cuda.synchronize()
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2):
        env.replay_sample(65, word, her=0.5, out=out)
    drawn = []
    for value in (2 ** 64 - 1, 0, 1):
        word.copy_(torch.tensor([value], dtype=torch.uint64))
        g2.replay()
        torch.cuda.synchronize()
        want = model.rows(65, value, 32768, 0)
        for f in rc.FIELDS:
            got = out[f].view(torch.uint8).cpu().numpy().view(rc.OUT_DTYPES[f]).reshape(want[f].shape)
            assert np.array_equal(got, want[f]), (value, f)
        drawn.append(out['slot'].clone() * n + out['env'])
    assert not torch.equal(drawn[0], drawn[1]) and not torch.equal(drawn[1], drawn[2])
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------ 6. the entry points
def test_errors_of_the_entry_points():
    from gym_craftingworld_amd import CraftingWorldVecEnv, _lib as L
    n, B = 8, 16
    env = CraftingWorldVecEnv(n, obs_mode='state', auto_reset=False, seed=3, **K5)
    lib, h, st = env._lib, env._h, env._stream()
    bufs = device_sentinels(B + 1)
    vp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    one = lambda **kw: L.cw_replay_out(**kw)  # noqa: E731
    full = one(**{f: vp(t) for f, t in bufs.items()})
    acts = torch.zeros(n, dtype=torch.int32, device='cuda')
    untouched = lambda: all(bool((t.view(torch.uint8) == SENT).all()) for t in bufs.values())  # noqa: E731
    assert lib.cw_replay_reserve(h, 4) == L.CW_OK                                 # (a buffer may be reserved before the first reset)
    assert lib.cw_replay_push(h, vp(acts), L.CW_ACT_I32, st) == L.CW_ERR_STATE and b'before cw_reset' in lib.cw_last_error()
    assert lib.cw_replay_sample(h, B, 0, None, 0, 0, C.byref(full), st) == L.CW_ERR_STATE and b'before cw_reset' in lib.cw_last_error()
    assert lib.cw_replay_clear(h, st) == L.CW_ERR_STATE
    assert lib.cw_replay_reserve(h, 0) == L.CW_OK
    env.reset()
    with pytest.raises(L.CraftingWorldError):                                     # no buffer, through the methods
        env.replay_push(acts)
    with pytest.raises(L.CraftingWorldError):
        env.replay_sample(B)
    tab = L.cw_replay_table()
    assert lib.cw_replay_buffers(h, C.byref(tab)) == L.CW_ERR_STATE and lib.cw_replay_bytes(h) == 0
    assert lib.cw_replay_clear(h, st) == L.CW_ERR_STATE and b'no buffer' in lib.cw_last_error()
    for steps in (-1, 2 ** 24 + 1, 2 ** 31 // n):
        assert lib.cw_replay_reserve(h, steps) == L.CW_ERR_INVALID
    env.replay_reserve(4)
    assert lib.cw_replay_bytes(h) == lib.cwh_replay_bytes_of(4, n) and lib.cw_replay_buffers(h, C.byref(tab)) == L.CW_OK and (tab.steps, tab.num_envs) == (4, n)
    assert lib.cw_replay_sample(h, B, 0, None, 65536, 0, C.byref(full), st) == L.CW_OK       # n = 0: no row is written
    assert lib.cw_replay_sample(h, 0, 0, None, 0, 0, C.byref(full), st) == L.CW_OK           # n_rows = 0: nothing enqueued
    torch.cuda.synchronize()
    assert untouched()
    a = (h, B, 0, None, 0, 0, C.byref(full))
    sub = lambda **kw: tuple(kw.get(k, v) for k, v in zip(('h', 'b', 'seed', 'seed_dev', 'her', 'strategy', 'out'), a))  # noqa: E731
    two = lambda f, g, off: C.byref(one(**{f: vp(bufs[f]), g: vp(bufs[f], off)}))  # noqa: E731
    invalid = [(sub(h=None), b'engine'), (sub(out=None), b'out'), (sub(b=-1), b'n_rows'), (sub(b=2 ** 27 + 1), b'n_rows'), (sub(her=65537), b'her'),
               (sub(strategy=2), b'strategy'), (sub(strategy=-1), b'strategy'), (sub(out=C.byref(one())), b'every field'),
               (sub(out=C.byref(one(hdr=vp(bufs['hdr'], 8)))), b'aligned'), (sub(out=C.byref(one(reward=vp(bufs['reward'], 2)))), b'aligned'),
               (sub(out=C.byref(one(desired=vp(bufs['desired'], 1)))), b'aligned'), (sub(out=C.byref(one(next_slot_pos=vp(bufs['next_slot_pos'], 4)))), b'aligned'),
               (sub(out=two('hdr', 'goal_hdr', 16 * (B - 1))), b'overlap'), (sub(out=two('reward', 'env', 4 * (B - 1))), b'overlap'),
               (sub(out=two('hdr', 'action', 16 * B - 1)), b'overlap'), (sub(out=two('slot', 'future', 0)), b'overlap')]
    for args, word in invalid:
        assert lib.cw_replay_sample(*args, st) == L.CW_ERR_INVALID, word
        assert word in lib.cw_last_error(), (word, lib.cw_last_error())
    assert lib.cw_replay_sample(*sub(out=two('hdr', 'goal_hdr', 16 * B)), st) == L.CW_OK     # (adjacent is not overlapping: the spare row)
    for args in ((None, vp(acts), L.CW_ACT_I32), (h, None, L.CW_ACT_I32), (h, vp(acts), 3), (h, vp(acts), -1)):
        assert lib.cw_replay_push(*args, st) == L.CW_ERR_INVALID                  # cw_step's argument rules
    torch.cuda.synchronize()
    assert untouched() and env.replay_size() == 0
    env.replay_push(acts)
    assert env.replay_size() == 1
    env.replay_clear()
    assert env.replay_size() == 0
    env.replay_push(acts)
    env.replay_reserve(0)                                                         # reserve(0), then push: no buffer
    assert lib.cw_replay_push(h, vp(acts), L.CW_ACT_I32, st) == L.CW_ERR_STATE and b'no buffer' in lib.cw_last_error()
    assert lib.cw_replay_sample(*a, st) == L.CW_ERR_STATE
    env.close()
