"""Writes tests/golden/ref_mip_lr.json: get_lr of the reference's own MipLrUpdaterHook (core/hooks/train_hooks.py, imported unmodified on
stubs: tests/runner_cases.reference_mip_lr_class) for the cases and iterations of tests/runner_cases.py.  Needs the reference tree."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import runner_cases as RC  # noqa: E402

if __name__ == '__main__':
    out = {'cases': RC.MIP_LR_CASES, 'iters': list(RC.MIP_LR_ITERS), 'lr': RC.mip_lr_values(RC.reference_mip_lr_class())}
    with open(RC.MIP_LR_GOLD, 'w') as f:
        json.dump(out, f, indent=1)
    print('wrote', RC.MIP_LR_GOLD, out['lr'])
