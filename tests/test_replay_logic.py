"""CPU tier: tests/replay_check.py itself -- the numpy ReplayModel on synthetic transitions: the episode rule and the ring worked out by hand, the draws of a
row against the library's own draw, the relabel against a row-by-row reading of the header, and the checkers against planted mistakes (each must be caught:
replay_check.FAULTS and a written sentinel row)."""
import numpy as np
import pytest

import replay_check as rc
from hostlib import host_lib

MAX_STEPS, TASK_MASK = 9, 0x1FF
SENT = 0xA5


def fresh(rng, n, subset):
    """n random records at the start of an episode: step_num 0, the reward rule in flag bit 1, achieved 0, a desired mask of the three low tasks"""
    h = rng.randint(0, 256, (n, 16)).astype(np.uint8)
    h[:, 4:6] = 0
    h[:, 6], h[:, 7] = rng.randint(0, 8, n), 0
    h[:, 8:12] = 0
    h[:, 10] = 2 * np.asarray(subset)
    return h, rng.randint(0, 2 ** 16, (n, 8)).astype(np.uint16)


class Walk:
    """synthetic envs: every push steps each env -- step_num up by one, achieved bits toggled when the step changes the state, reward and done by the
    step's own rule -- and afterwards a done env (auto-reset) and now and then another one (a discontinuity) starts over from a fresh record"""

    def __init__(self, n, seed, p_break=0.15):
        self.rng, self.n, self.p_break = np.random.RandomState(seed), n, p_break
        self.subset = np.arange(n) % 2
        self.hdr, self.pos = fresh(self.rng, n, self.subset)
        self.goal = fresh(self.rng, n, 0)

    def transition(self):
        rng, n = self.rng, self.n
        action = rng.randint(-2, 8, n)
        changed = (rng.rand(n) < 0.7) & (action >= 0) & (action <= 5)
        nh, npos = self.hdr.copy(), self.pos.copy()
        step = rc.u16(self.hdr, 8) + 1
        rc.put_u16(nh, 8, step)
        ach = np.where(changed, rc.u16(self.hdr, 4) ^ (1 << rng.randint(0, 3, n)), rc.u16(self.hdr, 4))
        rc.put_u16(nh, 4, ach)
        npos[changed, 0] += 1
        reward = rc.reward_rule(ach, rc.u16(self.hdr, 6), TASK_MASK, self.subset, changed, MAX_STEPS)
        done = (step >= MAX_STEPS) | (reward == MAX_STEPS)
        t = dict(hdr=self.hdr.copy(), slot_pos=self.pos.copy(), next_hdr=nh, next_slot_pos=npos, goal_hdr=self.goal[0].copy(), goal_slot_pos=self.goal[1].copy(),
                 action=action, reward=reward, done=done, changed=changed)
        again = done | (rng.rand(n) < self.p_break)
        fh, fp = fresh(rng, n, self.subset)
        self.hdr, self.pos = np.where(again[:, None], fh, nh), np.where(again[:, None], fp, npos)
        self.broke = again & ~done
        return t


def filled(L, n_envs, pushes, seed, fault=None):
    model, walk = rc.ReplayModel(L, n_envs, MAX_STEPS, TASK_MASK, fault), Walk(n_envs, seed)
    for _ in range(pushes):
        model.push(**walk.transition())
    return model


def test_the_draw_is_the_librarys():
    _, lib = host_lib()
    for seed in (0, 5, 2 ** 64 - 1):
        for b in (0, 1, 63, 999, 2 ** 27 - 1):
            for k in range(4):
                assert int(rc.draw(seed, b, k, 0)) == lib.cwh_shoot_draw_of(seed, b, k, 0)
    assert rc.mulhi32(2 ** 32 - 1, 70) == 69 and rc.mulhi32(0, 70) == 0 and rc.mulhi32(2 ** 31, 3) == 1


def test_the_episode_rule_and_the_ring_by_hand():
    """one env, L = 3: a continuing step, a done, a discontinuity, and the wrap -- the predecessor is the slot about to be overwritten when L = 1"""
    def push(model, s, s2, done=False):
        h, h2 = np.full((1, 16), s, np.uint8), np.full((1, 16), s2, np.uint8)
        z = np.zeros((1, 8), np.uint16)
        model.push(h, z, h2, z, h, z, [0], [-1], [done], [True])
    m = rc.ReplayModel(3, 1, MAX_STEPS, TASK_MASK)
    push(m, 1, 2)                       # position 0: episode 0
    push(m, 2, 3)                       # continues
    push(m, 3, 4, done=True)            # continues, and ends the episode
    assert m.buf['episode'][:, 0].tolist() == [0, 0, 0] and m.n == 3
    push(m, 4, 5)                       # the bytes continue, but the predecessor was done: episode 1, into slot 0
    push(m, 9, 10)                      # a discontinuity: episode 2
    assert m.buf['episode'][:, 0].tolist() == [1, 2, 0] and m.buf['hdr'][:, 0, 0].tolist() == [4, 9, 3] and m.env_episode.tolist() == [2] and m.n == 5
    m.clear()
    push(m, 10, 11)                     # the first push after a clear starts episode 0, whatever the slots hold
    assert m.n == 1 and m.buf['episode'][0, 0] == 0 and m.buf['hdr'][:, 0, 0].tolist() == [10, 9, 3]
    one = rc.ReplayModel(1, 1, MAX_STEPS, TASK_MASK)
    for s in (1, 2, 3):
        push(one, s, s + 1)
    assert one.buf['episode'][0, 0] == 0                     # L = 1: every push continues the one before it
    push(one, 7, 8)
    assert one.buf['episode'][0, 0] == 1
    wrong = rc.ReplayModel(1, 1, MAX_STEPS, TASK_MASK, fault='predecessor_after_write')
    for s in (1, 2, 3):
        push(wrong, s, s + 1)
    assert wrong.buf['episode'][0, 0] == 2                   # (read after the write, the slot never continues itself)


def test_out_of_range_actions_are_stored_as_255():
    m = rc.ReplayModel(2, 4, MAX_STEPS, TASK_MASK)
    z16, z8 = np.zeros((4, 16), np.uint8), np.zeros((4, 8), np.uint16)
    m.push(z16, z8, z16, z8, z16, z8, [-1, 5, 6, 2 ** 40], [-1] * 4, [False] * 4, [False] * 4)
    assert m.buf['action'][0].tolist() == [255, 5, 255, 255]


@pytest.mark.parametrize('L, pushes', [(1, 5), (3, 2), (3, 9), (8, 19)])
@pytest.mark.parametrize('strategy', [0, 1])
def test_the_rows_against_a_row_by_row_reading_of_the_header(L, pushes, strategy):
    n_envs, B, seed, her = 7, 300, 2 ** 63 + 11, 40000
    m = filled(L, n_envs, pushes, seed=L + pushes)
    rows = m.rows(B, seed, her, strategy)
    n, lo = m.n, max(0, m.n - L)
    for b in range(B):
        i = (int(rc.draw(seed, b, 0, 0)) * n_envs) >> 32
        p = lo + ((int(rc.draw(seed, b, 1, 0)) * (n - lo)) >> 32)
        relabel = (int(rc.draw(seed, b, 2, 0)) >> 16) < her
        assert (rows['env'][b], rows['slot'][b], bool(rows['relabel'][b])) == (i, p % L, relabel)
        assert lo <= p < n
        stored = {f: m.buf[f][p % L, i] for f in rc.BUFFER}
        if not relabel:
            for f in rc.RECORDS + ('action', 'reward'):
                assert np.array_equal(rows[f][b], stored[f]), f
            assert rows['done'][b] == (stored['flags'] >> 1) & 1 and rows['desired'][b] == rc.u16(stored['hdr'], 6) and rows['future'][b] == -1
            continue
        e = max(q for q in range(p, n) if all(m.buf['episode'][r % L, i] == stored['episode'] for r in range(p, q + 1)))
        f = e if strategy else p + ((int(rc.draw(seed, b, 3, 0)) * (e - p + 1)) >> 32)
        assert (rows['e'][b], rows['f'][b], rows['future'][b]) == (e, f, f % L)
        at_f = m.buf['next_hdr'][f % L, i]
        g = int(rc.u16(at_f, 4))
        assert rows['desired'][b] == g
        for k in ('hdr', 'next_hdr'):
            want = stored[k].copy()
            want[6], want[7] = g & 255, g >> 8
            assert np.array_equal(rows[k][b], want)
        want = at_f.copy()
        want[6], want[7] = g & 255, g >> 8
        assert np.array_equal(rows['goal_hdr'][b], want) and np.array_equal(rows['goal_slot_pos'][b], m.buf['next_slot_pos'][f % L, i])
        assert rc.u16(rows['goal_hdr'][b], 4) == rc.u16(rows['goal_hdr'][b], 6) == g
        a2, subset = int(rc.u16(stored['next_hdr'], 4)) & TASK_MASK, (stored['next_hdr'][10] >> 1) & 1
        gm = g & TASK_MASK
        hit = ((gm & ~a2) == 0 and (~(gm ^ a2) & TASK_MASK) != 0) if subset else a2 == gm
        reward = MAX_STEPS if (stored['flags'] & 1) and hit else -1
        assert rows['reward'][b] == reward and rows['done'][b] == int(rc.u16(stored['next_hdr'], 8) >= MAX_STEPS or reward == MAX_STEPS)
        assert np.array_equal(rows['slot_pos'][b], stored['slot_pos']) and rows['action'][b] == stored['action']


def test_an_empty_buffer_has_no_rows():
    m = rc.ReplayModel(4, 3, MAX_STEPS, TASK_MASK)
    assert m.rows(10, 0, 65536, 0) is None and m.coverage(None) == {}


# ---------------------------------------------------------------------------------------------------------------- the checkers and planted mistakes
L0, N0, PUSHES0, B0, SEED0 = 4, 9, 11, 400, 1234


def a_sample(model, B, seed, her, strategy, fields=rc.FIELDS):
    """what a correct call leaves: (before, after)"""
    before = rc.sentinels(B, SENT)
    rows = model.rows(B, seed, her, strategy)
    after = {f: (rows[f].copy() if f in fields and rows is not None else before[f].copy()) for f in rc.FIELDS}
    return before, after


def view_of(model):
    return dict({f: a.copy() for f, a in model.buf.items()}, env_episode=model.env_episode.copy(), n=np.array([model.n]))


@pytest.mark.parametrize('fields', [rc.FIELDS, ('reward', 'goal_hdr'), ('env',)])
def test_a_correct_sample_passes(fields):
    m = filled(L0, N0, PUSHES0, 3)
    for her, strategy in ((0, 0), (65536, 1), (32768, 0)):
        before, after = a_sample(m, B0, SEED0, her, strategy, fields)
        rows = rc.check_sample(m, B0, SEED0, her, strategy, before, after, fields)
        cov = m.coverage(rows)
        assert cov['relabelled'] == (0 if her == 0 else B0 if her == 65536 else cov['relabelled']) and cov['relabelled'] + cov['plain'] == B0
    empty = rc.ReplayModel(L0, N0, MAX_STEPS, TASK_MASK)
    before, after = a_sample(empty, 5, 0, 65536, 0)
    assert rc.check_sample(empty, 5, 0, 65536, 0, before, after) is None


def test_the_synthetic_buffer_covers_every_case():
    m = filled(L0, N0, PUSHES0, 3)
    cov = m.coverage(m.rows(B0, SEED0, 65536, 0))
    assert all(cov[k] > 0 for k in ('future_later', 'reward_max', 'miss_changed', 'miss_unchanged', 'cut_by_done', 'cut_by_break', 'crosses_wrap',
                                    'ends_newest')), cov


@pytest.mark.parametrize('fault', [f for f in rc.FAULTS if f != 'predecessor_after_write'])
def test_a_planted_mistake_in_the_sample_is_caught(fault):
    """the buffer is right, the rows are those of an implementation with one mistake: f drawn from [p + 1, e], e running past an episode end, a relabelled
    reward that ignores the changed gate, the subset rule swapped for the equal rule, done without its time-out term, bytes 6-7 not rewritten, lo off by
    one after a wrap"""
    good, bad = filled(L0, N0, PUSHES0, 3), filled(L0, N0, PUSHES0, 3, fault)
    rc.check_buffer(good, view_of(bad))                                # (the mistake is in the sample alone)
    caught = 0
    for strategy in (0, 1):
        before, after = a_sample(bad, B0, SEED0, 65536, strategy)
        try:
            rc.check_sample(good, B0, SEED0, 65536, strategy, before, after)
        except AssertionError:
            caught += 1
    assert caught >= (1 if fault in ('f_from_p_plus_1', 'subset_as_equal') else 2), fault      # (final never draws f; a proper subset needs a later f)


def test_the_predecessor_read_after_the_write_is_caught_at_L_1():
    good, bad, walk = rc.ReplayModel(1, N0, MAX_STEPS, TASK_MASK), rc.ReplayModel(1, N0, MAX_STEPS, TASK_MASK, 'predecessor_after_write'), Walk(N0, 8, p_break=0.0)
    with pytest.raises(AssertionError, match='episode'):
        for _ in range(4):
            t = walk.transition()
            bad.push(**t)
            rc.check_push(good, t, view_of(bad))


def test_a_push_that_touches_another_slot_or_forgets_n_is_caught():
    good, walk = rc.ReplayModel(3, N0, MAX_STEPS, TASK_MASK), Walk(N0, 9)
    for _ in range(4):
        t = walk.transition()
        after = rc.ReplayModel(3, N0, MAX_STEPS, TASK_MASK)
        after.buf, after.env_episode, after.n = {f: a.copy() for f, a in good.buf.items()}, good.env_episode.copy(), good.n
        after.push(**t)
        rc.check_push(good, t, view_of(after))
    t = walk.transition()
    for spoil, match in ((lambda v: v['reward'].__setitem__((0, 2), 77), 'reward'), (lambda v: v['n'].__setitem__(0, good.n), 'n = '),
                         (lambda v: v['flags'].__setitem__((good.n % 3, 1), 3 - v['flags'][good.n % 3, 1]), 'flags'),
                         (lambda v: v['env_episode'].__setitem__(4, v['env_episode'][4] + 1), 'env_episode')):
        trial = rc.ReplayModel(3, N0, MAX_STEPS, TASK_MASK)
        trial.buf, trial.env_episode, trial.n = {f: a.copy() for f, a in good.buf.items()}, good.env_episode.copy(), good.n
        after = rc.ReplayModel(3, N0, MAX_STEPS, TASK_MASK)
        after.buf, after.env_episode, after.n = {f: a.copy() for f, a in good.buf.items()}, good.env_episode.copy(), good.n
        after.push(**t)
        view = view_of(after)
        spoil(view)
        with pytest.raises(AssertionError, match=match):
            rc.check_push(trial, t, view)


def test_a_written_sentinel_is_caught():
    """a row written although the buffer is empty, and a field written that the call was not handed"""
    empty = rc.ReplayModel(L0, N0, MAX_STEPS, TASK_MASK)
    before, after = a_sample(empty, 6, 0, 0, 0)
    after['reward'][3] = -1
    with pytest.raises(AssertionError, match=r"sample\['reward'\], which the call must not write"):
        rc.check_sample(empty, 6, 0, 0, 0, before, after)
    m = filled(L0, N0, PUSHES0, 3)
    before, after = a_sample(m, B0, SEED0, 0, 0, ('hdr', 'reward'))
    after['future'][B0 - 1] = -1
    with pytest.raises(AssertionError, match=r"sample\['future'\], which the call must not write"):
        rc.check_sample(m, B0, SEED0, 0, 0, before, after, ('hdr', 'reward'))
    before, after = a_sample(m, B0, SEED0, 0, 0)
    after['hdr'][B0 - 1, 15] ^= 1
    with pytest.raises(AssertionError, match=r"sample\['hdr'\] differs at \(%d, 15\)" % (B0 - 1)):
        rc.check_sample(m, B0, SEED0, 0, 0, before, after)
