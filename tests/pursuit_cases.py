"""Case data and map builders that several Pursuit GPU test files share (a plain module, not collected): the crowd configurations and
free runs of test_pursuit_crowd_gpu.py and test_live_counts_crowd_gpu.py, their named maps, and the map kinds of step_to_twins.py."""
import numpy as np

from helpers import golden_id, pursuit_golden_files

CNN = dict(n_pursuers=100, n_evaders=300, obs_range=21, n_catch=2, surround=True, flatten=False, reward_mech="local")
SURROUND_24 = dict(n_pursuers=20, n_evaders=300, obs_range=9, n_catch=2, surround=True, flatten=True, reward_mech="local")
FREE_RUNS = {
    # name: (maps, config, envs, steps, max_steps, removed > 0, episodes ended by catches > 0)
    "cnn_rect128": ("rect128", CNN, 64, 60, 25, False, False),       # random pursuers surround nobody on 128 x 128: rows, moves, resets
    "cnn_pool128_sample_maps": ("pool128", dict(CNN, sample_maps=True), 64, 60, 25, False, False),
    "cnn_rows_48x48": ("rect48", CNN, 64, 60, 25, True, False),
    "surround_20v300": ("open24", SURROUND_24, 128, 60, 25, True, False),
    "colocate_global_260v40": ("open20", dict(n_pursuers=260, n_evaders=40, obs_range=5, n_catch=2, surround=False, flatten=True,
                                              reward_mech="global", catchr=0.1, urgency_reward=-0.05), 128, 120, 100, True, True),
    "surround_20v300_random_opponents": ("open24", dict(SURROUND_24, random_opponents=True, max_opponents=250), 128, 60, 25, True, False),
    "cnn_rows_48x48_constraint_window": ("rect48", dict(CNN, constraint_window=0.5), 64, 60, 25, True, False),
}


def golden(name):
    files = pursuit_golden_files()
    return np.load(files[[golden_id(p) for p in files].index(name)])


def named_maps(name):
    from madrl_amd.maps import rectangle_map, resize
    if name == "rect128":
        return [rectangle_map(128, 128)]
    if name == "pool128":   # ten 128 x 128 maps: resize(8, map_pool16) -- the authors' map_pool128.npy is not in their tree
        return list(resize(8, golden("pursuit_pool16_sample_maps")["maps"]))
    if name == "rect48":
        return [rectangle_map(48, 48)]
    if name == "open24":
        return [np.zeros((24, 24), np.int32)]
    if name == "open20":
        return [np.zeros((20, 20), np.int32)]
    raise KeyError(name)


def corridors(xs, ys):
    """rows 0 and xs - 1 free, everything between them built over: an agent never leaves its row, so the window cells beyond it stay
    outside the map (kept cells that survive every step and reset), and three agents on a cell are common"""
    m = np.full((xs, ys), -1, dtype=np.int32)
    m[0, :] = m[xs - 1, :] = 0
    return m


def maps(kind, xs, ys):
    """"rect": rectangle_map; "rect16": rectangle_map from 16 x 16 on, below that an all-free map; "pool": synthetic_map_pool(3, ...);
    "corridors": the map above"""
    from madrl_amd.maps import rectangle_map, synthetic_map_pool
    if kind == "rect16":
        kind = "rect" if min(xs, ys) >= 16 else "free"
    return {"pool": lambda: synthetic_map_pool(3, xs, ys), "rect": lambda: [rectangle_map(xs, ys)],
            "free": lambda: [np.zeros((xs, ys), np.int32)], "corridors": lambda: [corridors(xs, ys)]}[kind]()
