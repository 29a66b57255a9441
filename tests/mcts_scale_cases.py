"""The configurations of the thousand-game search tests, shared by the GPU tests (test_gpu_mcts_scale.py) and their CPU
companion (test_mcts_scale_cpu.py), which keeps them discriminating: a mix-up between games can only show if the games differ."""
from pyoracle import MCTS_DEFAULTS, coord

# A: lock step.  (n, G, rollouts, rollouts per batch, searches per game, nodes_per_game)
LOCKSTEP = [(9, 65, 16, 8, 3, 256),          # the second wave of the row scan
            (9, 1024, 8, 4, 2, 256),         # exactly one full chunk of the scan
            (9, 1025, 8, 4, 2, 256),         # one game into the second chunk
            (9, 2111, 12, 4, 3, 1024),       # a third, partial chunk, G no multiple of 64; 2 161 664 small ids > 8192 x 256
            (19, 1025, 8, 4, 2, 128)]        # the 19x19 node layout


def lockstep_cfg(G, roll, bs):
    cfg = dict(MCTS_DEFAULTS)
    cfg.update(num_games=G, rollouts_per_thread=roll, rollouts_per_batch=bs, seed=9001, net_salt=311, policy_distri_cutoff=6)
    return cfg


# B: evaluation games out of phase.  Black 16 rollouts at 8 per batch = 2 steps per move, White 12 at 4 = 3 steps; every odd game
# is put one forced move ahead, so even games start with Black's search and odd games with White's
UNEVEN_N, UNEVEN_G, UNEVEN_SEARCHES, UNEVEN_NODES = 9, 1100, 6, 256
UNEVEN_FORCED = coord(9, 2, 2)


def uneven_cfg(G=UNEVEN_G):
    cfg = dict(MCTS_DEFAULTS)
    cfg.update(num_games=G, rollouts_per_thread=16, rollouts_per_batch=8, white_rollouts_per_thread=12, white_rollouts_per_batch=4,
               seed=9001, net_salt=311, white_net_salt=312, black_ver=3, white_ver=4, policy_distri_cutoff=6)
    return cfg
