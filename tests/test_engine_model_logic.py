"""The CPU model of the batch engine (tests/engine_model.py) and the comparison of tests/test_call_sequences.py, themselves tested -- CPU only.
(a) the model runs the call-sequence scripts and every masked call, save and load of it is accepted by the per-call checkers that are pinned to the
reference already (masked_check.check_masked_call / untouched, snapshot_check.check_save / check_load); (b) a one-env model replays the op scripts of
the imagine fixtures captured from the reference: their goal states and stream positions; (c) a model with one defect is caught by the GPU tier's own
comparison at the first op the defect touches, and the message names that op."""
import numpy as np
import pytest

import engine_model as EM
import imagine_model as M
import sequence_script as SS
from engines import N1
from masked_check import check_masked_call, untouched
from oracle_replay import FRAMES, np_states
from snapshot_check import SKIPPED, check_load, check_save


def _model(kind, size, defect=None):
    model, _ = EM.model_for(kind, size, *np_states(N1, SS.BASE), defect=defect)
    model.snapshot_reserve(SS.CAP)
    return model


# ------------------------------------------------------------------------------------------------------------------------------ (a) the per-call checkers
def _full(rows, vals, N):
    """what an engine's output array holds: the selected rows written, the others as they were (zeros)"""
    out = np.zeros((N,) + vals.shape[1:], vals.dtype)
    out[rows] = vals
    return out


@pytest.mark.parametrize('kind,gap', [('state_auto_pool_menus', 0), ('pixels_alt_auto', 2), ('dirty_ray_auto', 0)])
def test_the_per_call_checkers_accept_the_model(kind, gap):
    ops = SS.script_of(kind, gap)
    model = _model(kind, 5)
    pixels, alt = kind != 'state_auto_pool_menus', kind == 'pixels_alt_auto'
    pending, rows_saved, checked = [], {}, dict.fromkeys(('imagine', 'imagine_commit', 'sample', 'reset_envs', 'save', 'load_stream', 'load_episode', 'ckpt_load'), 0)
    ckpt_takes = []
    for i, (name, args) in enumerate(ops):
        before = EM.as_take(model, pixels)
        pool = np.stack([e.fixed_states() for e in model.ora.envs]) if model.K else None
        out = EM.apply(model, name, args, pending)
        after = EM.as_take(model, pixels)
        tag = SS.describe(ops, i)
        try:
            if name in ('imagine', 'imagine_commit'):
                g, a = out['goal_grid'], out['goal_agent']
                oh = _full(out['rows'], np.stack([M.one_hot(g[j], a[j]) for j in range(len(g))]), N1)
                fr = _full(out['rows'], np.stack([M.render(g[j], a[j], alt) for j in range(len(g))]), N1) if pixels else None
                check_masked_call('imagine', before, after, args['mask'], desired=args['desired'], commit=name == 'imagine_commit', one_hot=oh, frames=fr,
                                  out_before=None, alt=alt)
            elif name == 'sample':
                check_masked_call('sample', before, after, args['mask'], cells=_full(out['rows'], out['cells'], N1), pool=pool if args['pooled'] else None)
            elif name == 'reset_envs':
                untouched(before, after, args['mask'])
                assert np.array_equal(after['counters'], before['counters'])
                sel = np.flatnonzero(args['mask'])
                assert (after['state_step_num'][sel] == 0).all() and (after['rng_pos'][sel] != before['rng_pos'][sel]).any()
            elif name == 'save':
                past = int((args['rows'] >= SS.CAP).sum())               # (the checker knows saves without a bad row: the count is checked here)
                assert after['counters'][SKIPPED] == before['counters'][SKIPPED] + past
                check_save(before, dict(after, counters=before['counters']))
                for e, r in enumerate(args['rows']):
                    if 0 <= r < SS.CAP:
                        rows_saved[int(r)] = {k: v[e].copy() for k, v in before.items() if k != 'counters'}
            elif name in ('load_stream', 'load_episode'):
                # check_load knows ONE save into an empty bank: the rows this load names, as if saved by envs 0, 1, ... at once, each as it was saved
                named = sorted(set(int(r) for r in args['rows'] if int(r) in rows_saved))
                save_rows = np.full(N1, -1, np.int32)
                save_rows[:len(named)] = named
                saved = {k: np.zeros_like(v) for k, v in before.items()}
                for j, r in enumerate(named):
                    for k, v in rows_saved[r].items():
                        saved[k][j] = v
                good, n_bad = check_load(saved, before, after, save_rows, args['rows'], name == 'load_stream', SS.CAP)
                assert np.array_equal(good, out['good']) and n_bad >= 1
            elif name == 'ckpt_save':
                ckpt_takes.append(before)
                continue
            elif name == 'ckpt_load':
                want = ckpt_takes.pop(0)
                for k in want:                                          # (the bank's count of skipped rows is not the checkpoint's)
                    assert np.array_equal(after[k][:4], want[k][:4]) if k == 'counters' else np.array_equal(after[k], want[k]), k
                assert after['counters'][SKIPPED] == before['counters'][SKIPPED]
            else:
                continue
        except AssertionError as err:
            raise AssertionError('%s: %s' % (tag, err)) from None
        checked[name] += 1
    assert min(checked.values()) >= len(SS.MUTATORS), checked


# ------------------------------------------------------------------------------------------------------------------------------ (b) the reference's op scripts
def _rng_cols(model):
    k, p = model.ora.envs[0].get_rng()
    return [int(p), M.crc(k)]


def _draw(model, n):
    """randint(n) from the env's stream, by numpy"""
    e = model.ora.envs[0]
    k, p = e.get_rng()
    rs = np.random.RandomState()
    rs.set_state(('MT19937', k, p, 0, 0.0))
    v = int(rs.randint(n))
    st = rs.get_state()
    e.set_rng(np.asarray(st[1], np.uint32), int(st[2]))
    return v


@pytest.mark.parametrize('name', M.fixture_names() + M.sweep_fixture_names())
def test_a_one_env_model_replays_the_imagine_fixtures(name):
    meta, kw, d = M.load(name)
    kw = dict(kw, alt_obs=meta['env'] == 'CraftingWorldEnvAltObs')
    kw.pop('stacked_obs', None)
    model = EM.EngineModel(1, d['key0'][None], [int(d['pos0'])], False, kw)
    S = kw.get('size', (21, 21))[0]
    states = []
    for i, (op, arg) in enumerate(zip(d['ops'].tolist(), d['args'].tolist())):
        want = d['rows'][i]
        tag = '%s op %d (%d, arg %d)' % (name, i, op, arg)
        if op == M.I_RESET:
            model.reset()
            got = [int(model.expected()['desired'][0])] + _rng_cols(model)
            assert got == want[:3].tolist(), tag
        elif op == M.I_STEP:
            r, dn = model.step([arg])
            a = model.expected()['agent_rc'][0]
            assert [int(r[0]), int(dn[0]), int(a[0]) * 256 + int(a[1])] == want[:3].tolist(), tag
        elif op == M.I_IMAGINE:
            x = model.expected()
            home = int(tuple(x['agent_rc'][0]) == tuple(x['init_agent_rc'][0]))
            used = int(x['desired'][0]) if arg < 0 else arg
            _, g, a = model.imagine_obs(None, None if arg < 0 else [arg])
            states.append((g[0], a[0]))
            got = [M.crc(g[0]), int(a[0][0]) * 256 + int(a[0][1])] + _rng_cols(model) + [used, home]
            assert got == want[[M.COL_STATE, M.COL_AGENT, M.COL_POS, M.COL_KEY, M.COL_DESIRED, M.COL_HOME]].tolist(), tag
            after = model.expected()
            assert all(np.array_equal(after[k], x[k]) for k in x if k not in ('rng_key', 'rng_pos')), tag      # (nothing committed)
        elif op in (M.I_SAMPLE, M.I_GENFIXED):
            if op == M.I_GENFIXED and not model.K:
                with pytest.raises(ValueError):
                    model.sample_states(None, pooled=True)
                assert [-1] + _rng_cols(model) == want[[0, M.COL_POS, M.COL_KEY]].tolist(), tag
                continue
            _, cells = model.sample_states(None, pooled=op == M.I_GENFIXED)
            codes, agent = M.codes_of_cells(S, cells[0])
            states.append((codes, agent))
            assert [M.crc(codes), agent[0] * 256 + agent[1]] + _rng_cols(model) == want[[M.COL_STATE, M.COL_AGENT, M.COL_POS, M.COL_KEY]].tolist(), tag
        elif op in (M.I_RANDINT, M.I_FOREIGN_RANDINT):                # (the caller's own RandomState IS the env's generator once assigned)
            assert _draw(model, arg) == want[0], tag
        elif op == M.I_ASSIGN:
            st = np.random.RandomState(arg).get_state()
            model.set_rng_states(np.asarray(st[1], np.uint32)[None], [int(st[2])])
        else:
            raise ValueError(op)
    assert len(states) > 20
    if 'state_codes' in d:
        assert np.array_equal(np.array([c for c, _ in states], np.uint8), d['state_codes'])
        assert np.array_equal(np.array([a for _, a in states], np.uint8), d['state_agent'])


# ------------------------------------------------------------------------------------------------------------------------------ (c) defects are caught at their op
TOUCHED_BY = {'load_takes_stream': ('load_episode',), 'reset_envs_keeps_stream': ('reset_envs',), 'commit_keeps_goal_grid': ('imagine_commit',),
              'set_state_ignores_step_num': ('set_phase',), 'skipped_not_counted': ('save', 'load_stream', 'load_episode')}


def _first_failure(kind, gap, defect, pixels):
    """the defective model in the engine's place, compared as tests/test_call_sequences.py compares -> (op index, message) of the first failure"""
    ops = SS.script_of(kind, gap)
    right, wrong = _model(kind, 5), _model(kind, 5, defect)
    pend_r, pend_w = [], []
    frames = tuple(FRAMES) if pixels else ()
    for i, (name, args) in enumerate(ops):
        EM.apply(right, name, args, pend_r)
        EM.apply(wrong, name, args, pend_w)
        try:
            EM.compare(wrong.expected(frames), wrong.counters, right)
        except AssertionError as err:
            return ops, i, SS.failure(kind, 5, gap, ops, i, '', err)
    return ops, None, ''


@pytest.mark.parametrize('defect', EM.DEFECTS)
@pytest.mark.parametrize('kind,gap', [('state_auto_pool_menus', 0), ('dirty_ray_auto', 2)])
def test_a_defect_is_caught_at_the_first_op_it_touches(kind, gap, defect):
    ops, at, msg = _first_failure(kind, gap, defect, kind == 'dirty_ray_auto')
    first = min(i for i, (name, _) in enumerate(ops) if name in TOUCHED_BY[defect])
    assert at == first, (at, first, msg)
    assert ('op %d:%s <- ' % (first, ops[first][0])) in msg and kind in msg and ('gap %d' % gap) in msg
    what = {'load_takes_stream': 'rng_', 'reset_envs_keeps_stream': 'rng_', 'commit_keeps_goal_grid': 'goal_grid', 'set_state_ignores_step_num': 'step_num',
            'skipped_not_counted': 'counters'}[defect]
    assert what in msg, msg


def test_a_right_model_passes_the_comparison():
    ops, at, msg = _first_failure('state_auto_pool_menus', 0, None, False)
    assert at is None, msg
