"""Deterministic evaluators on the device for the guided searches' GPU tests (tests/test_gpu_guided.py,
tests/test_gpu_bounce_guided.py, tests/test_gpu_guided_fuzz.py): plain torch functions of the leaves, with no
synchronisation, so that a step and its evaluation can be captured in a graph.  torch is imported inside the functions: the
module itself needs no GPU.  Not a test module."""


def torch_evaluator(grid, player):
    """a deterministic evaluator on the device: any function of the leaves will do, both callers see the same rows"""
    import torch

    x = grid.to(torch.float32)
    weights = torch.arange(1, grid.shape[1] * grid.shape[2] + 1, dtype=torch.float32, device=grid.device).view(1, grid.shape[1], grid.shape[2])
    priors = torch.softmax((x * weights).sum(dim=1) * 0.125, dim=1)
    values = torch.tanh((x * weights).sum(dim=(1, 2)) * 0.03125) * (1 - 2 * player.to(torch.float32))
    return priors.contiguous(), values.contiguous()


def torch_evaluator_moves(grid, player, targets):
    """a deterministic evaluator on the device: a softmax over the legal slots of `targets`, a value from the grid"""
    import torch

    n, h, w = grid.shape
    x = grid.to(torch.float32)
    weights = torch.arange(1, h * w + 1, dtype=torch.float32, device=grid.device).view(1, h, w)
    cells = torch.arange(h * w, device=grid.device, dtype=torch.int64).view(1, 1, h * w)
    legal = ((targets.view(n, w, 1) >> cells) & 1).bool()
    logits = (torch.arange(w, device=grid.device, dtype=torch.float32).view(1, w, 1) * 0.25
              + cells.to(torch.float32) * 0.0625 + (x * weights).sum(dim=(1, 2)).view(n, 1, 1) * 0.001)
    logits = torch.where(legal, logits, torch.full_like(logits, -1e30))
    priors = torch.softmax(logits.view(n, -1), dim=1).view(n, w, h * w) * legal
    values = torch.tanh((x * weights).sum(dim=(1, 2)) * 0.003) * (1 - 2 * player.to(torch.float32))
    return priors.contiguous(), values.contiguous()
