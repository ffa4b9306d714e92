"""GPU tier of the call sequences: every ordered pair of the engine's state-changing calls -- reset, reset_envs, imagine_obs with and without commit,
sample_states, snapshot_save, snapshot_load with and without the stream, set_state(step_num), set_rng_states, checkpoint save and load -- back to back
and with two steps between them (tests/sequence_script.py), on one engine per run that lives through the whole script.  After EVERY op the engine is
compared with the CPU model (tests/engine_model.py) through oracle_replay.same_states: every get_state() field, the three frames in the pixel modes,
every env's RNG key and position, counters 0-3 and 6, and what the op returned -- the rewards and dones of the steps, the goal frames or one-hot
states of an imagine, the cells of a sample.  The step segments go through step(), step_many(), a graph captured once before the script starts and
rollout(), as the script says; the manual engine steps and resets env.done.  A failure names the run, the op and the three ops before it.  Everything
is bit-exact.  No timing."""
import numpy as np
import pytest
import torch

import engine_model as EM
import imagine_model as M
import sequence_script as SS
from engines import K5, N1
from oracle_replay import FRAMES, make_env, np_states, same, snapshot

pytestmark = pytest.mark.gpu

SEGMENT = K5['max_steps'] + 2


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device='cuda')


def _variants(env, T):
    """the ways this engine can take T steps with every finished env reset"""
    if not env.auto_reset:
        return ['step_and_reset_envs']
    return ['step', 'step_many'] + (['graph'] if T == SEGMENT else []) + (['rollout'] if env.obs_mode == 'state' else [])


def _steps(env, graph, buf, args):
    """-> (how, rewards, dones): of every step where the variant shows them, else of the last one ([1, N])"""
    acts = _dev(args['actions'])
    T = acts.shape[0]
    ways = _variants(env, T)
    how = ways[args['variant'] % len(ways)]
    if how in ('step', 'step_and_reset_envs'):
        rs = torch.empty(acts.shape, dtype=torch.int32, device='cuda')
        ds = torch.empty(acts.shape, dtype=torch.bool, device='cuda')
        for t in range(T):
            _, r, d, _ = env.step(acts[t])
            rs[t], ds[t] = r, d
            if how == 'step_and_reset_envs':
                env.reset_envs(env.done)
    elif how == 'rollout':
        rs, ds = env.rollout(acts)
    else:
        if how == 'graph':
            buf.copy_(acts)
            graph.replay()
        else:
            env.step_many(acts)
        rs, ds = env.reward[None], env.done[None]
    torch.cuda.synchronize()
    return how, rs.cpu().numpy(), ds.cpu().numpy()


def _drive(env, name, args, pending, tmp_path, graph, buf, want, pixels):
    """one op on the engine, and what it returned against the model's `want` -> a word on how the op ran, for the failure message"""
    if name == 'steps':
        how, rew, done = _steps(env, graph, buf, args)
        same('reward of the steps', 0, rew.T, want['reward'][-len(rew):].T)
        same('done of the steps', 0, done.T, want['done'][-len(done):].T)
        return how
    if name == 'reset':
        env.reset()
    elif name == 'reset_envs':
        env.reset_envs(_dev(args['mask']))
    elif name in ('imagine', 'imagine_commit'):
        out = env.imagine_obs(_dev(args['mask']), desired=_dev(args['desired'].view(np.int16)), commit=name == 'imagine_commit', one_hot=not pixels)
        got, rows = out.cpu().numpy()[want['rows']], want['rows']
        g, a = want['goal_grid'], want['goal_agent']
        if pixels:
            same('goal frames', rows, got, np.stack([M.render(g[j], a[j], env.raster == 'alt') for j in range(len(rows))]))
        else:
            same('goal states', rows, got, np.stack([M.one_hot(g[j], a[j]) for j in range(len(rows))]))
    elif name == 'sample':
        cells = env.sample_states(_dev(args['mask']), pooled=args['pooled'])
        same('cells', want['rows'], cells.view(torch.int16).cpu().numpy().view(np.uint16)[want['rows']], want['cells'])
    elif name == 'save':
        env.snapshot_save(_dev(args['rows'], np.int32))
    elif name in ('load_stream', 'load_episode'):
        env.snapshot_load(_dev(args['rows'], np.int32), with_stream=name == 'load_stream')
    elif name == 'set_phase':
        env.set_state(step_num=args['phases'])
    elif name == 'set_rng':
        env.set_rng_states(*SS.rng_states(N1, args['base']))
    elif name == 'ckpt_save':
        pending.append(str(tmp_path / ('checkpoint_%d' % len(list(tmp_path.iterdir())))))
        env.save_checkpoint(pending[-1])
    elif name == 'ckpt_load':
        env.load_checkpoint(pending.pop(0))
    else:
        raise ValueError(name)
    return ''


def _compare(env, model, frames):
    EM.compare(snapshot(env, frames=frames), env._counters_raw.cpu().numpy(), model)


@pytest.mark.parametrize('kind,size,gap', SS.RUNS)
def test_every_pair_of_state_changing_calls_against_the_cpu_model(kind, size, gap, tmp_path):
    ops = SS.script_of(kind, gap)
    keys, pos = np_states(N1, SS.BASE)
    model, ekw = EM.model_for(kind, size, keys, pos)
    env, _, _ = make_env(N1, keys, pos, **ekw)
    try:
        pixels = env.obs_mode != 'state'
        frames = tuple(FRAMES) if pixels else ()
        assert env.tuner_state()['lookahead'] == (1 if env.auto_reset else 0)
        env.snapshot_reserve(SS.CAP)
        model.snapshot_reserve(SS.CAP)
        env.reset()                                               # (a capture needs an engine that has been reset; the script resets again)
        model.reset()
        buf = torch.zeros((SEGMENT, N1), dtype=torch.uint8, device='cuda')
        graph = env.capture_steps(buf) if env.auto_reset else None
        _compare(env, model, frames)
        pend_model, pend_env, ways = [], [], set()
        for i, (name, args) in enumerate(ops):
            how = ''
            try:
                want = EM.apply(model, name, args, pend_model)
                how = _drive(env, name, args, pend_env, tmp_path, graph, buf, want, pixels)
                _compare(env, model, frames)
            except AssertionError as err:
                raise AssertionError(SS.failure(kind, size, gap, ops, i, how, err)) from None
            ways.add(how)
        assert ways >= set(_variants(env, SEGMENT)), ways         # every step variant this engine has was used
    finally:
        env.close()
