"""What "a refit call did exactly what it should" means for cw_shoot_refit.  expected_elites() / expected_refit() are the numpy model, written from the text
of include/craftingworld.h alone: the elites by a STABLE argsort of the negated int64 column (return descending, sample ascending), sorted ascending; the
counts from shoot_check.model_actions(samples=elites), ALL T steps; the weights by the header's formula.  check_refit() compares every written row, the
untouched rows of the states that take no part, and ret and weights_in after the call.  columns() builds the inputs the GPU tier uses and split_ties() says
where a threshold value is shared by a chosen and an unchosen sample.  Pure CPU: numpy arrays in, no GPU.  A plain module, not a fixture;
tests/test_refit_logic.py tests the model and the comparison themselves."""
import numpy as np

from shoot_check import model_actions

FIELDS = ('elites', 'weights', 'elite_min')
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def weight(smooth, gain, count):
    """min(65535, smooth + gain * count) of the header, on integers or integer arrays (int64: nothing wraps, as nothing wraps in uint32)"""
    return np.minimum(65535, np.int64(smooth) + np.int64(gain) * np.asarray(count).astype(np.int64))


def expected_elites(ret, E):
    """ret integers [K, M] -> (elites int64 [E, M]: the first E samples of every column in the order (return descending, sample ascending), in ASCENDING
    sample order; elite_min int64 [M]: the smallest return among them)"""
    r = np.asarray(ret).astype(np.int64)
    first = np.argsort(-r, axis=0, kind='stable')[:E]                # (stable: among equal returns the smaller sample comes first)
    return np.sort(first, axis=0), np.take_along_axis(r, first[E - 1:E], axis=0)[0]


def expected_refit(ret, E, T, seed, weights_in=None, smooth=1, gain=1):
    """-> dict: elites [E, M], elite_min [M], counts [T, 6, M] (how many elites drew action a at step t: all T drawn actions) and weights [T, 6, M]; seed
    the EFFECTIVE seed (a Python int), weights_in None or integers [T, 6, M]"""
    K, M = np.shape(ret)
    elites, elite_min = expected_elites(ret, E)
    acts = model_actions(seed, M, K, T, weights_in, samples=elites)                      # [T, E, M]
    counts = np.stack([(acts == a).sum(axis=1) for a in range(6)], axis=1)               # [T, 6, M]
    assert (counts.sum(axis=1) == E).all()
    return dict(elites=elites, elite_min=elite_min, counts=counts, weights=weight(smooth, gain, counts))


def split_ties(ret, E):
    """bool [M]: the threshold value of the column is held by a chosen AND an unchosen sample -- where the tie rule decides something"""
    r = np.asarray(ret).astype(np.int64)
    _, v = expected_elites(r, E)
    return (E - (r > v[None]).sum(axis=0)) < (r == v[None]).sum(axis=0)


def takes_part(env_of, num_envs, M):
    """bool [M]: env_of None, or an entry in 0 .. num_envs - 1"""
    if env_of is None:
        return np.ones(M, bool)
    e = np.asarray(env_of).astype(np.int64)
    return (e >= 0) & (e < num_envs)


def _same(name, got, want, cols, what):
    got, want = np.asarray(got).astype(np.int64), np.asarray(want).astype(np.int64)
    assert got.shape == want.shape, '%s: shape %s, expected %s' % (name, got.shape, want.shape)
    bad = (got != want) & cols
    if bad.any():
        at = tuple(int(i) for i in np.argwhere(bad)[0])
        raise AssertionError('%s%s %s: got %d, expected %d (%d entries differ)' % (name, list(at), what, got[at], want[at], int(bad.sum())))


def check_refit(ret_before, ret_after, weights_in_before, weights_in_after, env_of, num_envs, E, T, seed, smooth, gain, before, after, *, in_place=False,
                want=None):
    """Pure CPU.  cw_shoot_refit ran between `before` and `after`, {field of FIELDS: the output buffer} (a field not asked for is absent from both).  ret
    [K, M] and weights_in (None or [T, 6, M]) as they were before and after the call, env_of (None or [M]) and num_envs, E, T, seed (the EFFECTIVE seed),
    smooth and gain as the call had them.  in_place: after['weights'] is the buffer weights_in was read from (weights_in_after is then not looked at).
    Asserts, in this order and naming the first entry that differs: ret is unchanged; weights_in is unchanged unless in place; of every state that takes
    part, elites (ascending, then equal to the model's), elite_min and weights equal expected_refit(); of every state that takes no part, every output
    holds what it held before.  want: expected_refit() of the same inputs, where a test has it already.  -> (states that took part, states that did not)."""
    K, M = np.shape(ret_before)
    everywhere = np.ones(M, bool)
    _same('ret', ret_after, ret_before, everywhere, 'was changed by the call')
    if weights_in_before is not None and not in_place:
        _same('weights_in', weights_in_after, weights_in_before, everywhere, 'was changed by a call that is not in place')
    assert set(before) == set(after) and set(after) <= set(FIELDS) and after, sorted(after)
    part = takes_part(env_of, num_envs, M)
    want = want or expected_refit(ret_before, E, T, seed, weights_in_before, smooth, gain)
    got = np.asarray(after['elites']).astype(np.int64) if 'elites' in after else None
    assert got is None or got.shape == (E, M), 'elites: shape %s, expected %s' % (got.shape, (E, M))
    if got is not None and E > 1:
        down = (np.diff(got, axis=0) <= 0) & part
        if down.any():
            e, j = (int(i) for i in np.argwhere(down)[0])
            raise AssertionError('elites[%d..%d, %d] not ascending: %d then %d' % (e, e + 1, j, got[e, j], got[e + 1, j]))
    for f in FIELDS:
        if f in after:
            _same(f, after[f], want[f], part, 'of a state that takes part')
            _same(f, after[f], before[f], ~part, 'of a state that takes no part was written')
    return int(part.sum()), int((~part).sum())


# ------------------------------------------------------------------------------------------------------------------------------ the columns the GPU tier uses
KINDS = ('equal', 'two', 'perm', 'extremes', 'lane')         # (the sixth kind, shoot()'s own returns, comes from shoot_check.recipe_shots / the card)
TIE_BEARING = ('equal', 'two', 'extremes', 'lane')           # kinds in which, for every K > E, some state's threshold value is held by a chosen and an unchosen sample


def columns(kind, K, M, E, seed=0):
    """int32 [K, M] of one kind:
    equal     one value everywhere;
    two       two values, the larger one held by (E + 1 + j) % (K + 1) samples of column j at random places: column 0 has E + 1 holders for E places;
    perm      K distinct values per column in random order, negative ones among them: no tie anywhere;
    extremes  INT32_MAX / 0 / INT32_MIN at random places, the counts chosen per column so that the threshold is 0 (columns 0, 1, 2 mod 5: E - 1 - j % 3 above
              it and j % 3 + 2 holders), INT32_MAX (3 mod 5: E + 1 holders) or INT32_MIN (4 mod 5), wherever K allows;
    lane      one value above the threshold on E - 1 samples, the threshold value on TWO neighbouring samples (one chosen, one not), the rest below, the
              pattern rotated from column to column -- by j where M >= K, so that every sample position, hence every lane and round, is once the chosen
              holder (but the last, which no rule can prefer to another) and once the unchosen one (but sample 0); spread evenly over 0 .. K - 1 where
              M < K."""
    rng = np.random.RandomState(1000 * K + 10 * E + seed)
    j = np.arange(M)
    if kind == 'equal':
        return np.full((K, M), -7, np.int32)
    if kind == 'perm':
        vals = (np.arange(K, dtype=np.int64) - K // 2) * 2000003 % (2 ** 31) - (np.arange(K) % 2) * 2 ** 30
        vals = np.unique(vals)
        assert len(vals) == K
        return vals[rng.rand(K, M).argsort(axis=0)].astype(np.int32)
    if kind == 'two':
        n_hi = (E + 1 + j) % (K + 1)
        sorted_cols = np.where(np.arange(K)[:, None] < n_hi[None], 5, -3)
    elif kind == 'extremes':
        n_max = np.select([j % 5 <= 2, j % 5 == 3], [np.maximum(0, E - 1 - j % 3), min(K, E + 1)], E // 3)
        n_zero = np.select([j % 5 <= 2, j % 5 == 3], [j % 3 + 2, 1], E // 3)
        n_zero = np.minimum(n_zero, K - n_max)
        k = np.arange(K)[:, None]
        sorted_cols = np.where(k < n_max[None], INT32_MAX, np.where(k < (n_max + n_zero)[None], 0, INT32_MIN))
    elif kind == 'lane':
        holders = 2 if K >= E + 1 else 1
        base = np.array([0] * holders + [-1] * (K - holders - (E - 1)) + [1] * (E - 1), np.int64)
        turn = j % K if M >= K else (j * K) // M
        return base[(np.arange(K)[:, None] - turn[None]) % K].astype(np.int32)
    else:
        raise ValueError(kind)
    return np.take_along_axis(np.broadcast_to(sorted_cols, (K, M)), rng.rand(K, M).argsort(axis=0), axis=0).astype(np.int32)


def shoot_columns(ret, M, E):
    """which M columns of shoot()'s returns [K, 600] a selection test of M states takes: the first M -- but for M = 1 the first column whose threshold value is
    held by a chosen and an unchosen sample (column 0 if there is none): one column of real returns may well have no tie to split"""
    if M == 1:
        split = np.flatnonzero(split_ties(ret, E))
        return split[:1] if len(split) else np.arange(1)
    return np.arange(M)
