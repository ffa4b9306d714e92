"""The oracle's full setter and copy (cwo_set_full, cwo_copy): what tests/engine_model.py builds snapshot rows, checkpoints and set_state from.  An env is
copied mid-episode and stepped beside the original across two resets: with the stream the copy is a twin for ever, without it the copy plays the copied
episode to its end and goes on with its own stream, pool and menu.  CPU only."""
import numpy as np
import pytest

from oracle import OracleEnv

KW = dict(size=(5, 5), max_steps=9)
MENU = dict(selected_tasks=['ChopTree', 'MoveAxe', 'EatBread', 'GoToHouse'], number_of_tasks=2)
EPISODE = ('grid', 'init_grid', 'goal_grid', 'agent', 'init_agent', 'goal_agent', 'hold', 'achieved', 'desired', 'step_num', 'ep_no', 'obs', 'desired_img',
           'init_img')
CONFIGS = {'ray': dict(), 'alt': dict(alt_obs=True), 'pool': dict(fixed_init_state=3)}


def _env(seed, **kw):
    st = np.random.RandomState(seed).get_state()
    return OracleEnv(rng_state=(np.asarray(st[1], np.uint32), int(st[2])), **dict(KW, **kw))


def _same(a, b, names, tag):
    sa, sb = a.state(), b.state()
    for k in names:
        assert np.array_equal(sa[k], sb[k]), '%s: %s' % (tag, k)


def _same_rng(a, b):
    (ka, pa), (kb, pb) = a.get_rng(), b.get_rng()
    return pa == pb and np.array_equal(ka, kb)


def _mid_episode(seed, **kw):
    """an env in its second episode, four steps in, holding something if the walk found it"""
    e = _env(seed, **kw)
    e.reset()
    for a in np.random.RandomState(seed + 1).randint(0, 6, KW['max_steps'] + 4):
        if e.step(int(a))[2]:
            e.reset()
    v = e.view()
    assert v.ep_no == 1 and 0 < v.step_num < KW['max_steps']
    return e


@pytest.mark.parametrize('config', list(CONFIGS))
def test_a_copy_with_the_stream_is_a_twin_across_two_resets(config):
    src = _mid_episode(40, **CONFIGS[config])
    dst = _env(41, **dict(CONFIGS[config], **MENU))               # another stream, another pool, another menu, never reset
    dst.copy_from(src, with_stream=True)
    assert dst.menu() == src.menu() and np.array_equal(dst.fixed_states(), src.fixed_states())
    resets = 0
    for t, a in enumerate(np.random.RandomState(42).randint(0, 6, 3 * KW['max_steps'])):
        (_, r1, d1, _), (_, r2, d2, _) = src.step(int(a)), dst.step(int(a))
        assert (r1, d1) == (r2, d2), t
        if d1:
            src.reset(), dst.reset()
            resets += 1
        _same(src, dst, EPISODE, 'step %d' % t)
        assert _same_rng(src, dst), t
    assert resets >= 2


@pytest.mark.parametrize('config', list(CONFIGS))
def test_a_copy_without_the_stream_plays_the_episode_and_goes_on_with_its_own(config):
    src = _mid_episode(50, **CONFIGS[config])
    dst, own = [_env(51, **dict(CONFIGS[config], **MENU)) for _ in range(2)]      # `own`: what dst's stream, pool and menu give by themselves
    rng0 = dst.get_rng()
    dst.copy_from(src, with_stream=False)
    assert _same_rng(dst, own) and np.array_equal(dst.get_rng()[0], rng0[0]) and dst.menu() == own.menu() != src.menu()
    assert np.array_equal(dst.fixed_states(), own.fixed_states())
    _same(src, dst, EPISODE, 'right after the copy')
    acts = np.random.RandomState(52).randint(0, 6, 3 * KW['max_steps'])
    first = None
    for t, a in enumerate(acts):
        (_, r1, d1, _), (_, r2, d2, _) = src.step(int(a)), dst.step(int(a))
        assert (r1, d1) == (r2, d2), t
        _same(src, dst, EPISODE, 'step %d, before the first reset' % t)
        if d1:
            first = t
            break
    assert first is not None
    ep = dst.view().ep_no
    dst.reset(), own.reset()                                       # the env's own stream from here on: `own` has drawn nothing but this reset either
    assert dst.view().ep_no == ep + 1
    resets = 1
    for t, a in enumerate(acts[first + 1:]):
        (_, r1, d1, _), (_, r2, d2, _) = own.step(int(a)), dst.step(int(a))
        assert (r1, d1) == (r2, d2), t
        if d1:
            own.reset(), dst.reset()
            resets += 1
        _same(own, dst, [k for k in EPISODE if k != 'ep_no'], 'step %d on the own stream' % t)
        assert _same_rng(own, dst), t
        assert dst.view().desired & ~0b001101010 == 0             # (only tasks of dst's own menu are drawn: bits 1, 3, 5, 6)
    assert resets >= 2


def test_set_full_sets_every_field_and_repaints_the_three_images():
    """the state of one env injected into another of another stream: equal views at once, the stream untouched, and equal steps up to the reset"""
    for kw in (dict(), dict(alt_obs=True)):
        src, dst = _mid_episode(60, **kw), _env(61, **kw)
        dst.reset()
        rng = dst.get_rng()
        st = src.state()
        dst.set_full(**{k: st[k] for k in EPISODE[:11]})
        _same(src, dst, EPISODE, 'after set_full')
        assert dst.get_rng()[1] == rng[1] and np.array_equal(dst.get_rng()[0], rng[0])
        dst.update(step_num=3)
        assert dst.view().step_num == 3
        _same(src, dst, [k for k in EPISODE if k != 'step_num'], 'after update(step_num)')
        dst.update(step_num=st['step_num'])
        for t, a in enumerate(np.random.RandomState(62).randint(0, 6, KW['max_steps'])):
            (_, r1, d1, _), (_, r2, d2, _) = src.step(int(a)), dst.step(int(a))
            assert (r1, d1) == (r2, d2), t
            _same(src, dst, EPISODE, 'step %d' % t)
            if d1:
                break
        assert d1


def test_bad_arguments_leave_the_env_untouched():
    e = _mid_episode(70)
    before = e.state()
    for bad in (dict(agent=(5, 0)), dict(hold=4), dict(goal_agent=(0, -1)), dict(grid=np.full((5, 5), 9, np.uint8))):
        with pytest.raises(ValueError):
            e.update(**bad)
    with pytest.raises(ValueError):
        e.copy_from(_env(71, size=(6, 6)))
    with pytest.raises(ValueError):
        e.copy_from(_env(72, fixed_init_state=2))
    after = e.state()
    for k in EPISODE:
        assert np.array_equal(before[k], after[k]), k
