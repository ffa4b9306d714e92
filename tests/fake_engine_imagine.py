"""tests/fake_engine.py's stand-in engine plus the two entry points the goal-drawing methods of the N=1 classes go through (CraftingWorldVecEnv.imagine_obs,
.sample_states), computed by the numpy model of tests/imagine_model.py on the oracle's state and stream -- TEST INFRASTRUCTURE ONLY."""
import numpy as np
import torch

import imagine_model as M
from fake_engine import FakeVecEnv


class FakeVecEnvImagine(FakeVecEnv):
    def _with_stream(self, fn):
        k, p = self._ora.get_rng()
        rs = np.random.RandomState()
        rs.set_state(('MT19937', k, p, 0, 0.0))
        out = fn(rs)
        st = rs.get_state()
        self._ora.set_rng(np.asarray(st[1], np.uint32), int(st[2]))
        return out

    def imagine_obs(self, mask=None, *, indices=None, desired=None, commit=False, out=None, one_hot=False):
        if not self._has_reset:
            raise RuntimeError('cw_imagine_masked called before cw_reset')
        assert mask is None and indices is None and not commit and out is None      # (what env.py asks for)
        s = self._ora.state()
        bits = int(s['desired']) if desired is None else int(np.asarray(desired).reshape(-1)[0])
        bits &= (1 << len(self.task_list)) - 1
        codes, agent = self._with_stream(lambda rs: M.imagine(s['init_grid'], s['init_agent'], s['agent'], bits, rs))
        res = M.one_hot(codes, agent) if one_hot else M.render(codes, agent, self._kw['alt_obs'])
        if not hasattr(self, '_imagine_scratch') or self._imagine_scratch.shape[1:] != res.shape:
            self._imagine_scratch = torch.zeros((1,) + res.shape, dtype=torch.uint8)       # engine-owned scratch, reused from call to call
        self._imagine_scratch[0] = torch.from_numpy(res)
        return self._imagine_scratch

    def sample_states(self, mask=None, *, indices=None, pooled=False):
        if not self._has_reset:
            raise RuntimeError('cw_sample_state_masked called before cw_reset')
        if pooled and not self.fixed_init_state:
            raise ValueError('sample_states(pooled=True) needs fixed_init_state > 0')
        cells = self._with_stream(lambda rs: M.generate_fixed_initial_state(self._ora.fixed_states(), rs) if pooled else M.sample_state(self.size, rs))
        if not hasattr(self, '_cells_scratch'):
            self._cells_scratch = torch.zeros((1, 9), dtype=torch.int16).view(torch.uint16)
        self._cells_scratch.numpy()[0] = cells
        return self._cells_scratch


def install(monkeypatch, resident=True):
    import gym_craftingworld_amd.env as E
    cls = type('FakeVecEnvImagine_%s' % ('resident' if resident else 'launch'), (FakeVecEnvImagine,), {'resident': resident})
    monkeypatch.setattr(E, 'CraftingWorldVecEnv', cls)
    monkeypatch.setattr(E, '_pinned_u8', lambda shape: torch.zeros(shape, dtype=torch.uint8))
    return cls
