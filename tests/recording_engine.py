"""A CraftingWorldVecEnv whose library only takes notes -- TEST INFRASTRUCTURE ONLY.

Most of vec_env.py is glue between Python arguments and the C ABI: which tensor's pointer reaches which parameter, what is packed on the host, what
is kept alive, when a host_outputs engine synchronises, what an empty batch of records does.  None of that needs a GPU to be WRONG.  `make_env()` builds
the object without its constructor (no engine, no device) on torch's CPU device and gives it RecordingLib below for a library: every entry point returns
0 and records (name, arguments) with the pointers as plain integers.  On the CPU device every host-validated path of a method runs up to the library
call; the in-place paths need `is_cuda` tensors and belong to the GPU tier, which wraps the real library in the same recorder
(tests/test_vec_env_calls_gpu.py).
"""
import ctypes as C

import torch

from gym_craftingworld_amd.vec_env import TASK_LIST, CraftingWorldVecEnv

_BYREF = type(C.byref(C.c_int()))
_NOT_RECORDED = ('cw_last_error', 'cw_snapshot_row_bytes')     # questions, not work


def _plain(a):
    """an argument as the test reads it: a pointer as its integer (None: NULL), a struct passed by reference as {field: value}"""
    if isinstance(a, C.c_void_p):
        return a.value
    if isinstance(a, _BYREF):
        return {f: getattr(a._obj, f) for f, _ in a._obj._fields_}
    return a


class RecordingLib:
    """stands in for (real=None) or in front of the loaded libcraftingworld.so: .calls lists (entry point, arguments after the engine handle)"""

    def __init__(self, real=None):
        self.calls, self._real = [], real

    def __getattr__(self, name):
        if not name.startswith('cw_'):
            raise AttributeError(name)

        def call(*args):
            if name not in _NOT_RECORDED:
                self.calls.append((name, tuple(_plain(a) for a in args[1:])))
            if self._real is not None:
                return getattr(self._real, name)(*args)
            return {'cw_snapshot_row_bytes': 64, 'cw_last_error': b'recording library'}.get(name, 0)
        return call

    def names(self):
        return [n for n, _ in self.calls]

    def clear(self):
        del self.calls[:]


def make_env(num_envs=4, size=5, host_outputs=False, fixed_init_state=0, snapshot_capacity=8):
    """what the methods under test read of an engine, and nothing else; call release(env) when done"""
    env = CraftingWorldVecEnv.__new__(CraftingWorldVecEnv)
    env.num_envs, env.size, env.device = num_envs, size, torch.device('cpu')
    env.frame_shape = (4 * size, 4 * size, 3)
    env.host_outputs, env.task_list, env.fixed_init_state = host_outputs, list(TASK_LIST), fixed_init_state
    env.obs_mode = 'state'
    env.hdr = torch.zeros((num_envs, 16), dtype=torch.uint8)
    env.achieved_mask = torch.zeros(num_envs, dtype=torch.int16)
    env.slot_pos = torch.zeros((num_envs, 8), dtype=torch.int16)
    env._h = C.c_void_p(1)
    env._stream = lambda: C.c_void_p(0)
    env._snapshot_capacity = snapshot_capacity
    env._keepalive = {}
    env._lib = RecordingLib()
    return env


def release(env):
    env._h = None          # (__del__ destroys nothing)


def kept_tensors(env):
    """{data_ptr: tensor} of every tensor the env references, directly or inside the tuples, lists and dicts it holds"""
    found = {}

    def walk(o):
        if torch.is_tensor(o):
            if o.data_ptr():
                found.setdefault(o.data_ptr(), o)
        elif isinstance(o, dict):
            for v in o.values():
                walk(v)
        elif isinstance(o, (tuple, list)):
            for v in o:
                walk(v)
    for v in vars(env).values():
        walk(v)
    return found
