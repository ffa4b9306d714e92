"""What "the replay calls did exactly what they should" means for cw_replay_push / cw_replay_sample: ReplayModel, a numpy model of the buffer written from
the text of include/craftingworld.h (the ring, THE EPISODE RULE, the draws of a row, the relabel), and check_push / check_sample, which compare the buffer
and the outputs of a call against it -- sentinel-filled outputs included: a row the call must not write and a field it was not handed keep their bytes.
draw() is tests/shoot_check.py's model of THE DRAW.  `fault=` makes the model behave like an implementation with one planted mistake
(tests/test_replay_logic.py: the checker must catch each).  Pure CPU: numpy arrays in, no GPU.  A plain module, not a fixture."""
import numpy as np

from shoot_check import draw

FIELDS = ('hdr', 'slot_pos', 'next_hdr', 'next_slot_pos', 'goal_hdr', 'goal_slot_pos', 'action', 'reward', 'done', 'desired', 'env', 'slot', 'future')
RECORDS = FIELDS[:6]
BUFFER = RECORDS + ('action', 'flags', 'reward', 'episode')
OUT_DTYPES = dict(hdr=np.uint8, slot_pos=np.uint16, next_hdr=np.uint8, next_slot_pos=np.uint16, goal_hdr=np.uint8, goal_slot_pos=np.uint16,
                  action=np.uint8, reward=np.int32, done=np.uint8, desired=np.uint16, env=np.int32, slot=np.int32, future=np.int32)
CHANGED, DONE = 1, 2
FAULTS = ('f_from_p_plus_1', 'e_past_episode_end', 'reward_ignores_changed', 'subset_as_equal', 'done_without_timeout', 'bytes_6_7_not_rewritten',
          'lo_off_by_one', 'predecessor_after_write')
_U = np.uint64


def row_shape(f):
    """what a row of output field f holds beyond its index: 16 header bytes, 8 slot positions, or one value"""
    return (16,) if f.endswith('hdr') else (8,) if f.endswith('slot_pos') else ()


def sentinels(B, byte=0xA5):
    """the 13 output buffers of a sample of B rows, every byte `byte`"""
    return {f: np.full((B,) + row_shape(f) + (np.dtype(dt).itemsize,), byte, np.uint8).view(dt).reshape((B,) + row_shape(f)) for f, dt in OUT_DTYPES.items()}


def mulhi32(a, b):
    return ((np.asarray(a, np.uint64) * np.asarray(b, np.uint64)) >> _U(32)).astype(np.int64)


def u16(hdr, at):
    """the little-endian uint16 at bytes at, at + 1 of headers uint8 [..., 16] -> int64"""
    return hdr[..., at].astype(np.int64) | hdr[..., at + 1].astype(np.int64) << 8


def put_u16(hdr, at, v):
    hdr[..., at], hdr[..., at + 1] = v & 0xFF, v >> 8


def reward_rule(achieved, goal, task_mask, subset, changed, max_steps):
    """the relabelled reward of the header on integer arrays: -1 unless changed; then max_steps iff the goal holds -- EQUAL: a == g, SUBSET: (g & ~a) == 0 and
    some position equal, all under the task mask"""
    a, g = np.asarray(achieved).astype(np.int64) & task_mask, np.asarray(goal).astype(np.int64) & task_mask
    hit = np.where(np.asarray(subset) != 0, ((g & ~a) == 0) & ((~(g ^ a) & task_mask) != 0), a == g)
    return np.where((np.asarray(changed) != 0) & hit, max_steps, -1).astype(np.int32)


def goal_record(goal_agent_rc, menu, desired, codes, goal_slot_pos):
    """THE GOAL RECORD of the header -> (goal_hdr uint8 [N, 16], goal_slot_pos uint16 [N, 8]); codes uint8 [N, 4], the goal state's slot codes"""
    n = len(menu)
    h = np.zeros((n, 16), np.uint8)
    h[:, 0:2], h[:, 3] = goal_agent_rc, menu
    put_u16(h, 4, np.asarray(desired).astype(np.int64))
    put_u16(h, 6, np.asarray(desired).astype(np.int64))
    h[:, 12:16] = codes
    return h, np.asarray(goal_slot_pos).view(np.uint16).reshape(n, 8).copy()


class ReplayModel:
    def __init__(self, steps, num_envs, max_steps, task_mask, fault=None):
        assert fault is None or fault in FAULTS
        self.L, self.N, self.max_steps, self.task_mask, self.fault = steps, num_envs, max_steps, task_mask, fault
        ln = (steps, num_envs)
        self.buf = {f: np.zeros(ln + ((16,) if f.endswith('hdr') else (8,)), OUT_DTYPES[f]) for f in RECORDS}
        self.buf.update(action=np.zeros(ln, np.uint8), flags=np.zeros(ln, np.uint8), reward=np.zeros(ln, np.int32), episode=np.zeros(ln, np.uint32))
        self.env_episode = np.zeros(num_envs, np.uint32)
        self.n = 0

    def clear(self):
        """n = 0, every env's episode number 0; the slots' bytes stay"""
        self.n = 0
        self.env_episode[:] = 0

    def push(self, hdr, slot_pos, next_hdr, next_slot_pos, goal_hdr, goal_slot_pos, action, reward, done, changed):
        """one push: the transitions of the N envs ([N, ...] each; slot_pos as int16 or uint16; action: any integers, outside 0..5 stored as 255) into slot
        n % L under THE EPISODE RULE"""
        rec = dict(hdr=hdr, slot_pos=slot_pos, next_hdr=next_hdr, next_slot_pos=next_slot_pos, goal_hdr=goal_hdr, goal_slot_pos=goal_slot_pos)
        rec = {f: np.ascontiguousarray(a).view(OUT_DTYPES[f]).reshape(self.buf[f].shape[1:]) for f, a in rec.items()}
        t = self.n % self.L
        done, changed, action = np.asarray(done).astype(bool), np.asarray(changed).astype(bool), np.asarray(action).astype(np.int64)
        if self.fault == 'predecessor_after_write':                   # (the slot is written first, then read back as the predecessor)
            prev = dict(next_hdr=rec['next_hdr'], next_slot_pos=rec['next_slot_pos'], done=done) if self.L == 1 else None
        else:
            prev = None
        if self.n == 0:
            ep = np.zeros(self.N, np.uint32)
        else:
            q = (self.n - 1) % self.L
            p_next_hdr, p_next_pos, p_done = self.buf['next_hdr'][q], self.buf['next_slot_pos'][q], (self.buf['flags'][q] & DONE) != 0
            if prev is not None:
                p_next_hdr, p_next_pos, p_done = prev['next_hdr'], prev['next_slot_pos'], prev['done']
            goes_on = ~p_done & (p_next_hdr == rec['hdr']).all(axis=1) & (p_next_pos == rec['slot_pos']).all(axis=1)
            ep = (self.env_episode + np.where(goes_on, 0, 1).astype(np.uint32)).astype(np.uint32)
        for f in RECORDS:
            self.buf[f][t] = rec[f]
        self.buf['action'][t] = np.where((action < 0) | (action > 5), 255, action)
        self.buf['flags'][t] = np.where(changed, CHANGED, 0) | np.where(done, DONE, 0)
        self.buf['reward'][t] = reward
        self.buf['episode'][t] = ep
        self.env_episode[:] = ep
        self.n += 1

    def rows(self, B, seed, her, strategy):
        """the B rows of cw_replay_sample(B, seed, her, strategy) -> dict: the 13 output fields, and relabel, p, e, f (positions; e, f = -1 where the row is
        not relabelled), changed (the stored bit); None for an empty buffer"""
        n, L, N = self.n, self.L, self.N
        if n == 0:
            return None
        lo = max(0, n - L)
        if self.fault == 'lo_off_by_one' and n > L:
            lo += 1
        V = n - lo
        b = np.arange(B)
        i = mulhi32(draw(seed, b, 0, 0), N)
        p = lo + mulhi32(draw(seed, b, 1, 0), V)
        relabel = (draw(seed, b, 2, 0) >> _U(16)).astype(np.int64) < her
        ep = self.buf['episode']
        e = p.copy()
        if self.fault == 'e_past_episode_end':
            e[:] = n - 1
        else:
            live = np.ones(B, bool)
            for k in range(1, L):
                q = p + k
                live &= (q < n) & (ep[np.minimum(q, n - 1) % L, i] == ep[p % L, i])
                e += live
        r3 = draw(seed, b, 3, 0)
        if strategy == 1:
            f = e.copy()
        elif self.fault == 'f_from_p_plus_1':
            f = np.where(e > p, p + 1 + mulhi32(r3, np.maximum(e - p, 1)), p)
        else:
            f = p + mulhi32(r3, e - p + 1)
        sp, sf = p % L, f % L
        out = {k: self.buf[k][sp, i].copy() for k in RECORDS}
        flags = self.buf['flags'][sp, i]
        changed = (flags & CHANGED) != 0
        g = u16(self.buf['next_hdr'][sf, i], 4)
        a_next = u16(out['next_hdr'], 4)
        subset = (out['next_hdr'][:, 10] >> 1) & 1
        if self.fault == 'subset_as_equal':
            subset = np.zeros_like(subset)
        new_reward = reward_rule(a_next, g, self.task_mask, subset, np.ones(B, bool) if self.fault == 'reward_ignores_changed' else changed, self.max_steps)
        timed_out = u16(out['next_hdr'], 8) >= self.max_steps
        new_done = (new_reward == self.max_steps) | (timed_out & (self.fault != 'done_without_timeout'))
        r = relabel
        goal_h = self.buf['next_hdr'][sf, i].copy()
        put_u16(goal_h, 6, g)
        out['goal_hdr'] = np.where(r[:, None], goal_h, out['goal_hdr'])
        out['goal_slot_pos'] = np.where(r[:, None], self.buf['next_slot_pos'][sf, i], out['goal_slot_pos'])
        if self.fault != 'bytes_6_7_not_rewritten':
            for k in ('hdr', 'next_hdr'):
                h = out[k].copy()
                put_u16(h, 6, g)
                out[k] = np.where(r[:, None], h, out[k])
        out['action'] = self.buf['action'][sp, i]
        out['reward'] = np.where(r, new_reward, self.buf['reward'][sp, i]).astype(np.int32)
        out['done'] = np.where(r, new_done, (flags & DONE) != 0).astype(np.uint8)
        out['desired'] = np.where(r, g, u16(self.buf['hdr'][sp, i], 6)).astype(np.uint16)
        out['env'], out['slot'] = i.astype(np.int32), sp.astype(np.int32)
        out['future'] = np.where(r, sf, -1).astype(np.int32)
        out.update(relabel=r, p=p, e=np.where(r, e, -1), f=np.where(r, f, -1), changed=changed)
        return out

    def coverage(self, rows):
        """what a sample's rows exercise, counted from the model alone -> dict of counts (tests/test_replay.py asserts its own coverage with it)"""
        if rows is None:
            return {}
        r, p, e, f, n, L = rows['relabel'], rows['p'], rows['e'], rows['f'], self.n, self.L
        i = rows['env'].astype(np.int64)
        rew = rows['reward']
        end_done = (self.buf['flags'][np.maximum(e, 0) % L, i] & DONE) != 0
        return dict(relabelled=int(r.sum()), plain=int((~r).sum()), future_later=int((r & (f > p)).sum()),
                    reward_max=int((r & (rew == self.max_steps)).sum()), miss_changed=int((r & (rew == -1) & rows['changed']).sum()),
                    miss_unchanged=int((r & (rew == -1) & ~rows['changed']).sum()), cut_by_done=int((r & (e < n - 1) & end_done).sum()),
                    cut_by_break=int((r & (e < n - 1) & ~end_done).sum()), crosses_wrap=int((r & (e % L < p % L)).sum()),
                    ends_newest=int((r & (e == n - 1)).sum()))


def _same(got, want, what):
    got, want = np.ascontiguousarray(got), np.asarray(want)
    assert got.shape == want.shape, '%s: shape %s, expected %s' % (what, got.shape, want.shape)
    if got.dtype.itemsize == want.dtype.itemsize and got.dtype != want.dtype:
        got = got.view(want.dtype)
    bad = np.argwhere(got != want)
    assert not len(bad), '%s differs at %s: got %s, expected %s (%d entries differ)' % (what, tuple(int(x) for x in bad[0]), got[tuple(bad[0])], want[tuple(bad[0])], len(bad))


def check_buffer(model, view, what='buffer'):
    """the engine's buffer (replay_view() as numpy: BUFFER, 'env_episode', 'n') against the model: every slot, written or not"""
    assert int(np.asarray(view['n']).reshape(-1)[0]) == model.n, '%s: n = %d, expected %d' % (what, int(np.asarray(view['n']).reshape(-1)[0]), model.n)
    for f in BUFFER:
        _same(view[f], model.buf[f], '%s[%r]' % (what, f))
    _same(view['env_episode'], model.env_episode, '%s[env_episode]' % what)


def check_push(model, transition, view_after):
    """one push: the model takes `transition` (ReplayModel.push's arguments as a dict) and the buffer afterwards must be the model's, byte for byte --
    the slot written, every other slot untouched, the episode numbers, n advanced by one"""
    model.push(**transition)
    check_buffer(model, view_after, 'after push %d' % (model.n - 1))


def check_sample(model, B, seed, her, strategy, before, after, fields=FIELDS):
    """one sample: before / after hold all 13 output buffers [B, ...] as numpy (sentinel-filled before the call); `fields` are those the call was handed.
    A field handed over holds the model's rows (or, with an empty buffer, what it held); every other field is untouched.  -> the model's rows"""
    want = model.rows(B, seed, her, strategy)
    for f in FIELDS:
        if f in fields and want is not None:
            _same(after[f], want[f], 'sample[%r]' % f)
        else:
            _same(after[f], before[f], 'sample[%r], which the call must not write,' % f)
    return want
