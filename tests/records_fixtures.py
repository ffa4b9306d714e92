"""The synthetic engine the four tests/test_*_logic.py of the records calls share: five oracle envs some steps into their episodes, a take()-shaped snapshot
of them, and the env_of every one of them hands in.  Pure CPU.  A plain module, not a fixture."""
import numpy as np

from records_check import encode

N, S, SENT = 5, 5, 0xA5
ENV_OF = np.array([0, 4, -1, 2, 2, 7, 1, -7, 3, 5 + 31, 0, 2 ** 31 - 1], np.int64)       # 12 states: 7 take part (env 2 and 0 twice), 2 take none, 3 are skipped
M = len(ENV_OF)


def world():
    """N oracle envs of max_steps 9 some steps into their episodes -> (dense states [N], their init grids)"""
    from oracle import OracleEnv
    rng = np.random.RandomState(5)
    st = []
    for i in range(N):
        o = OracleEnv(size=(S, S), max_steps=9)
        o.seed_int(100 + i)
        o.reset()
        for a in rng.randint(0, 6, 4 + i):
            o.step(int(a))
        st.append(o.state())
    dense = dict(grid=np.stack([s['grid'] for s in st]), agent=np.array([s['agent'] for s in st]), hold=np.array([s['hold'] for s in st]),
                 achieved=np.array([s['achieved'] for s in st]), desired=np.array([s['desired'] for s in st]),
                 step_num=np.array([min(s['step_num'], 9 - 2) for s in st]), flags=np.array([2 * (i % 2) for i in range(N)]))
    return dense, np.stack([s['init_grid'] for s in st])


def snap(dense, init_grids):
    """a take()-shaped snapshot of the N envs (what check_records_call reads of it, and some buffers it must find unchanged)"""
    hdr, pos = encode(dense, menu=3)
    r = np.random.RandomState(2)
    return dict(state_grid=dense['grid'].copy(), state_init_grid=init_grids.copy(), rng_pos=r.randint(1, 625, N).astype(np.int32),
                rng_key=r.randint(0, 2 ** 31, (N, 624)).astype(np.uint32), hdr=hdr, slot_pos=pos.view(np.int16), reward=np.full(N, -1, np.int32),
                done=np.zeros(N, bool), counters=np.arange(8, dtype=np.int64) * 11)
