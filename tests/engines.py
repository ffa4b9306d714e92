"""The engine configurations the GPU tiers share: the 70-env engines of the snapshot, expand, simulate, plan and shoot tests, the grid sizes they run at,
and the card's CU count, which the launch rules are written in.  A plain module, not a fixture."""
import numpy as np

K5 = dict(size=(5, 5), max_steps=17)
SIZES = [5, 4, 7, 8, 21]              # 7 / 8: the full-frame engine changes painter (gather up to 7, piece sweep from 8); 21: the headline frame
N1 = 70
MENUS = [dict(), dict(selected_tasks=['ChopTree', 'MoveAxe', 'EatBread', 'GoToHouse'], number_of_tasks=2)]      # (the same reward rule: with_stream=False keeps the row's)
ENGINES = {'state_manual': dict(obs_mode='state', auto_reset=False),
           'dirty_ray_auto': dict(obs_mode='pixels_dirty', raster='ray'),
           'pixels_alt_auto': dict(obs_mode='pixels', raster='alt'),
           'state_auto_pool_menus': dict(obs_mode='state', fixed_init_state=3, task_menus=MENUS, env_menu=(np.arange(N1) % 2).astype(np.uint8))}


def k_of(S):
    """the configuration of the round-trip and expand tests at size S: max_steps stays 17, so 2 * 17 + 3 steps reset every env twice at any size"""
    return dict(K5, size=(S, S))


def n_cu():
    import torch
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
