"""Trajectory.paths(): episode segments are cut on the terminal and time-limit bits of the done bytes (no GPU needed)."""
import torch


def test_paths_cut_on_episode_boundaries_only():
    """bit 7 of a done byte (a capacity overflow mark of PursuitEvade / MultiWalker) is no episode boundary"""
    from madrl_amd.rollout import Trajectory
    dones = torch.tensor([[0, 128], [1, 128], [0, 2], [128, 0]], dtype=torch.uint8)
    z = torch.zeros((4, 2, 1))
    tr = Trajectory(actions=z.clone(), rewards=z.clone(), returns=z.clone(), dones=dones, advantages=None, observations=None)
    cuts = sorted((d["env_id"], len(d["rewards"]), d["terminated"]) for d in tr.paths())
    assert cuts == [(0, 2, False), (0, 2, True), (1, 1, False), (1, 3, True)]
