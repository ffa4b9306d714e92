"""CPU tier: from load_records()'s Python arguments to cw_load_records' parameters, through the recording engine (tests/recording_engine.py: the library
only takes notes) -- the envs / src pairing, what is packed and kept alive, the host-side refusals -- and the pure packing functions of vec_env.py.  The
in-place hand-over needs device tensors: tests/test_load_records.py wraps the real library in the same recorder."""
import numpy as np
import pytest
import torch

from gym_craftingworld_amd.vec_env import load_records_args, load_records_src
from load_records_check import MUTATIONS, good_record, mutated, record_rule
from recording_engine import kept_tensors, make_env, release

S, N = 5, 4


def _records(n, bad=None):
    hdr, pos = np.stack([good_record(S)[0] for _ in range(n)]), np.stack([good_record(S)[1] for _ in range(n)])
    hdr[:, 8] = np.arange(n)                                    # step_num tells the records apart
    if bad is not None:
        hdr[bad], pos[bad] = mutated('two held', S)
    return hdr, pos


# ------------------------------------------------------------------------------------------------------------------------------ the pure functions
def test_src_alone_holds_one_entry_per_env():
    assert load_records_src(4, 4).tolist() == [0, 1, 2, 3]
    assert load_records_src(4, 9, [8, -1, -7, 0]).tolist() == [8, -1, -1, 0]
    assert load_records_src(4, 9, np.array([3, 3, 3, 3], np.int16)).tolist() == [3, 3, 3, 3]          # any number of envs may name one record
    out = load_records_src(4, 0, [-1, -1, -1, -1])
    assert out.dtype == np.int32 and out.flags['C_CONTIGUOUS'] and out.tolist() == [-1] * 4
    for src, n in (([0, 1, 2], 9), (None, 3), ([[0, 1], [2, 3]], 9), ([0.0, 1.0, 2.0, 3.0], 9), ([True, False, True, False], 9)):
        with pytest.raises(ValueError):
            load_records_src(4, n, src)
    for src in ([0, 1, 2, 9], [2 ** 31 - 1, 0, 0, 0]):
        with pytest.raises(IndexError, match='outside 9 records'):
            load_records_src(4, 9, src)


def test_envs_are_paired_with_records():
    assert load_records_src(6, 2, [0, 1], envs=[3, 5]).tolist() == [-1, -1, -1, 0, -1, 1]
    assert load_records_src(6, 2, envs=[5, 3]).tolist() == [-1, -1, -1, 1, -1, 0]                     # without src: envs[j] takes record j
    assert load_records_src(6, 2, [1, 1, -4], envs=[-1, 0, 2]).tolist() == [1, -1, -1, -1, -1, 1]
    assert load_records_src(6, 2, [], envs=[]).tolist() == [-1] * 6
    for src, envs in (([0], [1, 2]), ([0, 1], [2, 2]), ([0, 1], [2, -4]), ([0, 1], [[1], [2]]), ([0, 1], [1.0, 2.0])):
        with pytest.raises(ValueError):
            load_records_src(6, 2, src, envs)
    for envs in ([6, 0], [-7, 0]):
        with pytest.raises(IndexError, match='outside a batch of 6'):
            load_records_src(6, 2, [0, 1], envs)
    with pytest.raises(IndexError, match='record index 2 outside 2 records'):
        load_records_src(6, 2, [0, 2], envs=[1, 3])


def test_records_are_validated_through_the_rule_and_packed():
    hdr, pos = _records(6)
    h, p, idx = load_records_args(N, S, hdr.reshape(2, 3, 16), pos.reshape(2, 3, 8).view(np.int16), [5, -1, 0, 0])
    assert h.dtype == np.uint8 and h.shape == (6, 16) and p.dtype == np.uint16 and p.shape == (6, 8) and idx.tolist() == [5, -1, 0, 0]
    assert h.flags['C_CONTIGUOUS'] and p.flags['C_CONTIGUOUS'] and np.array_equal(h, hdr) and np.array_equal(p, pos)
    seen = []
    load_records_args(N, S, hdr, pos, [5, -1, 0, 0], record_ok=lambda s, a, b: seen.append((s, int(a[8]))) or True)
    assert seen == [(S, 0), (S, 5)]                             # every record some env takes, once; no other
    for name in MUTATIONS:                                      # the library's rule is the default
        hdr[2], pos[2] = mutated(name, S)
        with pytest.raises(ValueError, match='record 2 cannot be loaded'):
            load_records_args(N, S, hdr, pos, [0, 1, 2, 3])
        assert load_records_args(N, S, hdr, pos, [0, 1, -1, 3])[2].tolist() == [0, 1, -1, 3]      # a bad record nobody takes is nobody's business
    hdr, pos = _records(6, bad=1)
    hdr[4], pos[4] = mutated('code 9', S)
    with pytest.raises(ValueError, match='record 1 cannot'):    # the FIRST bad record
        load_records_args(N, S, hdr, pos, [4, 1, 0, 0])
    with pytest.raises(ValueError, match='record 3 '):
        load_records_args(N, S, *_records(6), [3, 0, 0, 0], record_ok=lambda s, a, b: record_rule(s, a, b) and a[8] != 3)
    for h, p in ((hdr[:, :15], pos), (hdr, pos[:, :7]), (hdr[:5], pos), (hdr.astype(np.int32), pos), (hdr, pos.astype(np.int32)), (None, pos), (hdr, None)):
        with pytest.raises(ValueError):
            load_records_args(N, S, h, p, [0, 0, 0, 0])
    with pytest.raises(IndexError):
        load_records_args(N, S, *_records(6), [6, 0, 0, 0])
    with pytest.raises(ValueError, match='one entry per env'):
        load_records_args(N, S, *_records(6))


# ------------------------------------------------------------------------------------------------------------------------------ through the method
@pytest.fixture
def env():
    e = make_env(num_envs=N, size=S)
    yield e
    release(e)


def _the_call(env):
    calls = [c for c in env._lib.calls if c[0] == 'cw_load_records']
    assert len(calls) == 1 and env._lib.names() == ['cw_load_records']
    return calls[0][1]


def _at(env, ptr, dtype, shape):
    t = kept_tensors(env)[ptr]
    assert t.dtype == dtype and tuple(t.shape) == shape and t.is_contiguous()
    return t.numpy()


def test_the_method_hands_over_records_src_and_status(env):
    hdr, pos = _records(6)
    obs, status = env.load_records(hdr, pos, [5, -1, 0, 0], status=True)
    assert set(obs) == {'hdr', 'slot_pos'} and obs['hdr'] is env.hdr
    src_p, hdr_p, pos_p, n, status_p, stream = _the_call(env)
    assert n == 6 and not stream and status_p == status.data_ptr() and status.dtype == torch.uint8 and tuple(status.shape) == (N,)
    assert np.array_equal(_at(env, hdr_p, torch.uint8, (6, 16)), hdr)
    assert np.array_equal(_at(env, pos_p, torch.int16, (6, 8)).view(np.uint16), pos)
    assert _at(env, src_p, torch.int32, (N,)).tolist() == [5, -1, 0, 0]


def test_the_method_pairs_envs_with_records_and_takes_tensors(env):
    hdr, pos = _records(2)
    out = env.load_records(torch.as_tensor(hdr), torch.as_tensor(pos.view(np.int16)), torch.as_tensor([1, 0]), envs=[3, 1])
    assert isinstance(out, dict)
    src_p, hdr_p, pos_p, n, status_p, _ = _the_call(env)
    assert n == 2 and status_p is None and _at(env, src_p, torch.int32, (N,)).tolist() == [-1, 0, -1, 1]
    env._lib.clear()
    env.load_records(*_records(N))                              # neither src nor envs: record i for env i
    src_p, _, _, n, _, _ = _the_call(env)
    assert n == N and _at(env, src_p, torch.int32, (N,)).tolist() == [0, 1, 2, 3]


def test_the_method_refuses_on_the_host_before_any_call(env):
    hdr, pos = _records(6, bad=2)
    for call, err in ((lambda: env.load_records(hdr, pos, [0, 2, 0, 0]), ValueError), (lambda: env.load_records(hdr, pos, [0, 6, 0, 0]), IndexError),
                      (lambda: env.load_records(hdr, pos), ValueError), (lambda: env.load_records(hdr, None), ValueError),
                      (lambda: env.load_records(hdr, pos, [0, 1], envs=[1, 1]), ValueError), (lambda: env.load_records(hdr, pos, [0, 1], envs=[4, 1]), IndexError),
                      (lambda: env.load_records(hdr[:, :8], pos, [0, 0, 0, 0]), ValueError)):
        with pytest.raises(err):
            call()
    assert env._lib.calls == []
    env.load_records(hdr, pos, [0, -1, 1, 5])                   # the bad record is not named: the call goes out
    assert env._lib.names() == ['cw_load_records']


def test_no_records_no_call(env):
    obs, status = env.load_records(np.zeros((0, 16), np.uint8), np.zeros((0, 8), np.int16), [-1] * N, status=True)
    assert env._lib.calls == [] and status.tolist() == [0] * N
