"""Time of TrainStep.step on the s1 fixture of tests/test_gpu_train_step.py (profiles/drop_grad.md, section 3):

    python tools/drop_grad_step_time.py <repository root> <off|on>       -> one STEP line
"""
import importlib
import os
import statistics
import sys

import torch

root, mode = os.path.abspath(sys.argv[1]), sys.argv[2]
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, 'tests'))
pkg = importlib.import_module('cvpr2025-decafnet_amd')
import step_grad_ref as R  # noqa: E402
from test_gpu_train_step import batch_of, opt_of  # noqa: E402

f = R.Fixture('s1')
opt = opt_of(pkg, f)
if mode == 'on':
    for part in ('vid_net', 'fusion'):
        opt.model[part]['proj_pdrop'] = opt.model[part]['path_pdrop'] = 0.1
model = pkg.modeling.PtTransformerEarlyFusionIterative(opt, second_fusion=False)
model.load_state_dict(f.sd)
model = model.cuda()
if mode == 'on':
    model.enable_dropout(seed=11)
ts = pkg.train.TrainStep(model, opt, itrs_per_epoch=1)
batch, targets = batch_of(f)
for _ in range(5):
    ts.step(batch, targets)
torch.cuda.synchronize()
times = []
for _ in range(30):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    ts.step(batch, targets)
    b.record()
    b.synchronize()
    times.append(a.elapsed_time(b))
times.sort()
print(f'STEP {os.path.basename(root) or root} dropout {mode}: median {statistics.median(times):.3f} ms, min {times[0]:.3f}, p90 {times[26]:.3f} (30 steps after 5)')
