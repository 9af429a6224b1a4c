"""Cases of the gradient fixture (tests/golden/objective_grad.npz) that tests/objective_cases.py does not hold: the loss-function
grid, the constructed non-smooth pairs and the extreme logits.  Shared by the generator and the tests."""
import itertools

import torch

# ---- the loss functions on their own
LOSS_SEED = 777
LOSS_N = 96
REDUCTIONS = ('none', 'sum', 'mean')
SELECTS = (False, True)
FOCAL_GRID = list(itertools.product((-1.0, 0.5), (2.0, 1.5), (True, False)))        # alpha, gamma, smoothing
IOU_KINDS = ('giou', 'diou')


def loss_inputs():
    """logits, (smoothed) targets, predicted and ground-truth offsets, a selection mask; tie-free by construction (random reals)"""
    g = torch.Generator().manual_seed(LOSS_SEED)
    x = torch.randn(LOSS_N, generator=g) * 3.0
    t = (torch.rand(LOSS_N, generator=g) < 0.3).float() * 0.8 + 0.1
    pred = torch.rand(LOSS_N, 2, generator=g) * 6.0
    gt = torch.rand(LOSS_N, 2, generator=g) * 6.0 + 0.05
    sel = torch.rand(LOSS_N, generator=g) < 0.6
    up = torch.randn(LOSS_N, generator=g)                                             # upstream gradient of reduction 'none'
    return x, t, pred, gt, sel, up


UP_SCALAR = 0.75                                                                      # upstream gradient of 'sum' / 'mean'

# ---- the non-smooth points: the four pairs of the convention table (include/decafnet_hip.h) and their mirror images
TIE_PRED = [[2.0, 3.0], [0.0, 1.0], [0.0, 0.0], [0.0, 0.0], [3.0, 2.0], [1.0, 0.0], [0.0, 0.0]]
TIE_GT = [[2.0, 3.0], [0.0, 2.0], [0.0, 0.0], [1.0, 2.0], [3.0, 2.0], [2.0, 0.0], [2.0, 1.0]]
# d ctr_diou_loss(reduction='sum') / d pred under eager autograd, rows 0 - 3 as stated in the table
TIE_DIOU_EAGER = {0: [0.0, 0.0], 1: [-0.03125, -0.625], 2: [-5e7, -5e7]}

# ---- extreme logits: |x| = 20, 100 against both smoothed labels
EXTREME_X = [20.0, -20.0, 100.0, -100.0, 20.0, -20.0, 100.0, -100.0]
EXTREME_POS = [True, True, True, True, False, False, False, False]


def key(*parts):
    return '/'.join(str(int(p)) if isinstance(p, bool) else str(p) for p in parts)
