"""CPU tier: what CraftingWorldVecEnv.plan hands to the library -- entry point, scalars, which pointer sits in which slot, the NULL members of fields not
named, what comes back, what an empty batch does, what raises before any call and what is kept alive (tests/recording_engine.py: the env without an engine,
a library that takes notes), after tests/test_vec_env_calls.py."""
import numpy as np
import pytest
import torch

from gym_craftingworld_amd.vec_env import PLAN_FIELDS
from recording_engine import make_env, release
from test_vec_env_calls import LEAD, M, N, S, at, packed, raises_before_any_call, records, the_call

KERNEL = PLAN_FIELDS[:7]
DEFAULT = ('q', 'length', 'done', 'achieved_mask', 'plan', 'best_action', 'best_q')
MEMBER = {'achieved_mask': 'achieved'}          # the out dict's key -> the member of cw_plan_out


@pytest.fixture(params=[False, True], ids=['device_outputs', 'host_outputs'])
def env(request):
    e = make_env(N, S, host_outputs=request.param)
    yield e
    release(e)


def shapes(D, m, names):
    spec = {'q': ((6, m), torch.int32), 'length': ((6, m), torch.int32), 'done': ((6, m), torch.bool), 'achieved_mask': ((6, m), torch.int16),
            'hdr': ((6, m, 16), torch.uint8), 'slot_pos': ((6, m, 8), torch.int16), 'plan': ((6, D, m), torch.uint8), 'best_action': ((m,), torch.uint8),
            'best_q': ((m,), torch.int32)}
    return {f: spec[f] for f in names}


def check_out(out, want, struct, scratch_q=False):
    """the returned dict against the spec, and the struct the library got: a kernel field's member holds its tensor's pointer, every other member is NULL
    (scratch_q: but q, which best_action / best_q are derived from, points at a tensor of the env's own)"""
    assert list(out) == list(want) and {f: (tuple(t.shape), t.dtype) for f, t in out.items()} == want
    assert list(struct) == ['q', 'length', 'done', 'achieved', 'hdr', 'slot_pos', 'plan']
    for f in KERNEL:
        got = struct[MEMBER.get(f, f)]
        if f in out:
            assert got == out[f].data_ptr(), f
        elif f == 'q' and scratch_q:
            assert got is not None
        else:
            assert got is None, f


def test_plan_with_records(env):
    h, p = records()
    r = env.plan(3, h, p, [0, 1, 2, 3, -5, 0])
    e, hp, pp, m, depth, struct = the_call(env, 'cw_plan')
    assert (m, depth) == (M, 3)
    packed(env, e, torch.int32, [0, 1, 2, 3, -1, 0])
    assert at(env, hp).dtype == torch.uint8 and tuple(at(env, hp).shape) == LEAD + (16,)
    assert at(env, pp).dtype == torch.int16 and tuple(at(env, pp).shape) == LEAD + (8,)
    check_out(r, shapes(3, M, DEFAULT), struct)                  # the default: everything but the records
    assert struct['hdr'] is None and struct['slot_pos'] is None
    assert env.plan(3, h, p, fields=DEFAULT, out=r) is r         # an earlier call's dict, written again
    e, hp, pp, m, depth, struct = the_call(env, 'cw_plan')
    assert e is None and (m, depth) == (M, 3)
    check_out(r, shapes(3, M, DEFAULT), struct)
    full = env.plan(8, h, p.view(np.uint16), fields=PLAN_FIELDS)
    struct = the_call(env, 'cw_plan')[5]
    check_out(full, shapes(8, M, PLAN_FIELDS), struct)
    assert all(v is not None for v in struct.values())


def test_plan_of_the_engines_own_states(env):
    own = env.plan(np.int64(2))
    e, hp, pp, m, depth, struct = the_call(env, 'cw_plan')
    assert (e, hp, pp, m, depth) == (None, None, None, N, 2)
    check_out(own, shapes(2, N, DEFAULT), struct)


def test_fields_not_named_are_null(env):
    h, p = records()
    r = env.plan(4, h, p, fields=('q', 'hdr'))
    struct = the_call(env, 'cw_plan')[5]
    check_out(r, shapes(4, M, ('q', 'hdr')), struct)
    assert [k for k, v in struct.items() if v is None] == ['length', 'done', 'achieved', 'slot_pos', 'plan']
    r = env.plan(4, h, p, fields=('plan',))
    struct = the_call(env, 'cw_plan')[5]
    check_out(r, shapes(4, M, ('plan',)), struct)
    assert [k for k, v in struct.items() if v is not None] == ['plan']


def test_best_action_without_q_reads_a_scratch_q(env):
    """best_action and best_q are derived from q: when q itself is not asked for the kernel still writes one, into a tensor the env keeps alive"""
    h, p = records()
    r = env.plan(2, h, p, fields=('best_action', 'length'))
    struct = the_call(env, 'cw_plan')[5]
    check_out(r, shapes(2, M, ('best_action', 'length')), struct, scratch_q=True)
    q = at(env, struct['q'])
    assert q.dtype == torch.int32 and tuple(q.shape) == (6, M) and [k for k, v in struct.items() if v is None] == ['done', 'achieved', 'hdr', 'slot_pos', 'plan']


def test_best_action_is_the_smallest_maximiser(env):
    """the reduction itself, on a q the test writes through out= (the recording library writes nothing): ties go to the SMALLEST action"""
    h, p = records()
    out = env.plan(2, h, p, fields=('q', 'best_action', 'best_q'))
    env._lib.clear()
    q = torch.tensor([[-2, 5, -2, 7, -2, -2], [-2, 5, -2, 3, -2, 16], [-2, -9, 4, 7, -2, 16], [-2, 5, 4, 7, -2, -2], [-2, 5, 4, 7, -3, 16], [-2, 5, 4, 6, -1, 16]],
                     dtype=torch.int32)
    out['q'].copy_(q)
    assert env.plan(2, h, p, fields=('q', 'best_action', 'best_q'), out=out) is out
    the_call(env, 'cw_plan')
    assert out['best_q'].tolist() == [-2, 5, 4, 7, -1, 16] and out['best_action'].tolist() == [0, 0, 2, 0, 5, 1]
    assert out['best_action'].dtype == torch.uint8 and out['best_q'].dtype == torch.int32


@pytest.mark.parametrize('lead', [(0,), (0, 3)])
def test_no_records_no_call(env, lead):
    h, p = records(lead)
    r = env.plan(5, h, p, fields=PLAN_FIELDS)
    assert {f: (tuple(t.shape), t.dtype) for f, t in r.items()} == shapes(5, 0, PLAN_FIELDS)
    assert env.plan(5, h, p, [], fields=PLAN_FIELDS, out=r) is r
    assert env._lib.calls == []


def test_errors_before_any_call(env):
    h, p = records()
    r = env.plan(3, h, p, fields=PLAN_FIELDS)
    env._lib.clear()
    for depth in (0, 9, -1, 2.0, '3', None, True):
        raises_before_any_call(env, ValueError, env.plan, depth, h, p)
        raises_before_any_call(env, ValueError, env.plan, depth)
    raises_before_any_call(env, ValueError, env.plan, 8, *records((2558,)))                      # 2 558 x 6^8 > 2^32
    raises_before_any_call(env, ValueError, env.plan, 6, *records((92057,)))
    for fields in ((), ('q', 'nope'), ('q', 'q'), ('reward',), ('ret',)):
        raises_before_any_call(env, ValueError, env.plan, 3, h, p, fields=fields)
    raises_before_any_call(env, ValueError, env.plan, 3, h)                                       # hdr without slot_pos
    raises_before_any_call(env, ValueError, env.plan, 3, None, p)
    raises_before_any_call(env, ValueError, env.plan, 3, env_of=[0, 1, 2, 3])                     # env_of without records
    raises_before_any_call(env, ValueError, env.plan, 3, h, p[:1])
    raises_before_any_call(env, ValueError, env.plan, 3, h.astype(np.int8), p)
    raises_before_any_call(env, ValueError, env.plan, 3, h, p, [0, 1, 2])
    raises_before_any_call(env, IndexError, env.plan, 3, h, p, [0, 1, 2, 3, 4, 0])
    raises_before_any_call(env, ValueError, env.plan, 3, h, p, fields=PLAN_FIELDS, out={f: r[f] for f in ('q', 'done')})
    raises_before_any_call(env, ValueError, env.plan, 3, h, p, fields=PLAN_FIELDS, out=dict(r, extra=r['q']))
    raises_before_any_call(env, ValueError, env.plan, 3, h, p, out=r)                             # (the default fields are not the dict's)
    raises_before_any_call(env, ValueError, env.plan, 4, h, p, fields=PLAN_FIELDS, out=r)         # the depth is part of plan's shape
    for f, bad in (('q', torch.empty((6, M + 1), dtype=torch.int32)), ('q', torch.empty((6, M), dtype=torch.int64)), ('done', torch.empty((6, M), dtype=torch.uint8)),
                   ('hdr', torch.empty((6, M, 32), dtype=torch.uint8)[:, :, ::2]), ('slot_pos', np.empty((6, M, 8), np.int16)),
                   ('plan', torch.empty((6, M, 3), dtype=torch.uint8)), ('best_action', torch.empty((M,), dtype=torch.int64)),
                   ('best_q', torch.empty((6, M), dtype=torch.int32))):
        raises_before_any_call(env, ValueError, env.plan, 3, h, p, fields=PLAN_FIELDS, out=dict(r, **{f: bad}))
