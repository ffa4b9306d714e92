"""EngineModel (tests/engine_model.py) with the one call it lacks: load_records -- TEST INFRASTRUCTURE ONLY.  A record is decoded
(records_check.decode) and injected into the oracle env with OracleEnv.update: the current state, hold, both masks and step_num are the record's, the
episode -- start and goal states, ep_no, stream, pool, menu -- stays the env's.  Which envs load is load_records_check.expected_status: the rule written
from the header's text, not the library's.  pairs_script() is the short script of tests/test_load_records.py: load_records before and after every
state-changing call of tests/sequence_script.py's circuit, and after itself."""
import numpy as np

import sequence_script as SS
from engine_model import EngineModel
from load_records_check import BAD_INDEX, LOADED, REFUSED, dense_of, expected_status, mutated
from records_check import decode, encode
from snapshot_check import SKIPPED


class LoadRecordsModel(EngineModel):
    def records(self, flags=0):
        """every env's current state as a packed record (hdr uint8 [N, 16], slot_pos uint16 [N, 8]); the menu byte is 0"""
        return encode(dense_of(self.ora.envs, flags))

    def load_records(self, hdr, slot_pos, src=None):
        """env i takes record src[i] (None: record i) -> the status bytes; an index out of range and a refused record are skipped and counted"""
        S = self.ora.envs[0].size
        hdr, pos = np.asarray(hdr, np.uint8).reshape(-1, 16), np.ascontiguousarray(slot_pos).reshape(-1, 8).view(np.uint16)
        status, src = expected_status(self.N, len(hdr), S, hdr, pos, src)
        good = np.flatnonzero(status == LOADED)
        if len(good):
            d = decode(hdr[src[good]], pos[src[good]], S)
            for j, i in enumerate(good.tolist()):
                self.ora.envs[i].update(grid=d['grid'][j], agent=d['agent'][j], hold=int(d['hold'][j]), achieved=int(d['achieved'][j]),
                                        desired=int(d['desired'][j]), step_num=int(d['step_num'][j]))
        self.counters[SKIPPED] += int(((status == BAD_INDEX) | (status == REFUSED)).sum())
        return status


def model_for(kind, size, keys, pos):
    """engine_model.model_for with the extended model -> (model, the engine's own kwargs)"""
    from engines import ENGINES, MENUS, N1, k_of
    from oracle_replay import oracle_kw
    ekw = dict(dict(ENGINES, pixels_ray_auto=dict(obs_mode='pixels', raster='ray'))[kind])
    kw = oracle_kw(dict(k_of(size), fixed_init_state=ekw.get('fixed_init_state', 0)), ekw.get('raster', 'ray'))
    per_env = [MENUS[int(m)] for m in ekw['env_menu']] if 'env_menu' in ekw else None
    return LoadRecordsModel(N1, keys, pos, ekw.get('auto_reset', True), kw, per_env), dict(ekw, **k_of(size))


def load_src(rs, N, R):
    """the src of one load op: a fork (a seventh of the envs from one record), records in a drawn order over half of the envs, and among the rest -7, R and
    R + 3; every other env takes no part"""
    src = np.full(N, -1, np.int32)
    envs = rs.permutation(N)
    fork, perm = N // 7, N // 2
    src[envs[:fork]] = int(rs.randint(R))
    src[envs[fork:fork + perm]] = rs.permutation(R)[np.arange(perm) % R]
    src[envs[fork + perm:fork + perm + 3]] = (-7, R, R + 3)
    return src


def pairs_script(seed, N, max_steps, S, pooled=False):
    """-> a list of (name, args): an opening walk and an 'archive' op (the model's states become the records), then for every mutator m of
    sequence_script.MUTATORS the ops m, 'load_records' and 'load_records', m -- each pair followed by two steps, a checkpoint loaded right behind the pair
    that saved it --, 'load_records' twice, an 'archive' refreshed halfway, and 2 * max_steps + 3 closing steps.  The records of a load are the archive's
    with one refused record (a mutation of load_records_check.MUTATIONS) written over record 0."""
    rs = np.random.RandomState(seed)
    steps = lambda T: ('steps', dict(actions=rs.randint(0, 6, (T, N)).astype(np.uint8), variant=0))  # noqa: E731
    saved = set()

    def mutator(name):
        """the op `name` with arguments drawn as sequence_script.build draws them"""
        if name == 'reset_envs':
            return name, dict(mask=SS._mask(rs, N))
        if name in ('imagine', 'imagine_commit'):
            return name, dict(mask=SS._mask(rs, N), desired=rs.randint(0, 512, N).astype(np.uint16))
        if name == 'sample':
            return name, dict(mask=SS._mask(rs, N), pooled=bool(pooled))
        if name == 'save':
            rows = SS._save_rows(rs, N)
            saved.update(rows[(rows >= 0) & (rows < SS.CAP)].tolist())
            return name, dict(rows=rows)
        if name in ('load_stream', 'load_episode'):
            return name, dict(rows=SS._load_rows(rs, N, saved))
        if name == 'set_phase':
            return name, dict(phases=rs.randint(0, max_steps, N).astype(np.int32))
        if name == 'set_rng':
            return name, dict(base=int(rs.randint(1, 2 ** 20)))
        return name, {}

    def load():
        return ('load_records', dict(src=load_src(rs, N, N), bad=mutated('two held', S)))
    ops = [('reset', {}), steps(9), ('archive', {})]
    for k, m in enumerate(SS.MUTATORS):
        for pair in ((m, None), (None, m)):
            for x in pair:
                ops.append(load() if x is None else mutator(x))
            if m == 'ckpt_save':
                ops.append(('ckpt_load', {}))
            ops.append(steps(2))
        if k == len(SS.MUTATORS) // 2:
            ops.append(('archive', {}))
    ops += [load(), load(), steps(2 * max_steps + 3)]
    return ops
