"""KiloNeRF distillation at Lego scale on one GPU: per-iteration times of the example generator, the teacher query (the 8 x 256
NerfMLP on 512 x 128 examples) and the fused student step (xr_kilo_student_step with Adam), the student step's plain-PyTorch
`bmm` restatement (forward + autograd backward + torch.optim.Adam) on the same data, and the occupancy grid at [144, 256, 160] x 27
points.  python tools/microbench_kilo_distill.py [--iters N]; run under `rocprofv3 --kernel-trace --stats -- python ...` for the
per-kernel summary (profiles/)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3            # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--skip-occupancy', action='store_true')
    args = ap.parse_args()
    from xrnerf_amd import kilo_distill as KD
    from xrnerf_amd.vanilla import NerfMLP
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))
    from test_gpu_kilo_distill import bmm_reference, bmm_params
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    gmin, gmax = [-0.67, -1.2, -0.37], [0.67, 1.2, 1.03]
    dmin, dmax = KD.fixed_resolution_domains(gmin, gmax, [9, 16, 10])
    dmin, dmax = dmin[:512].to(dev), dmax[:512].to(dev)
    teacher = NerfMLP(embedder=dict(type='BaseEmbedder', i_embed=0, multires=10, multires_dirs=4, input_ch=3)).to(dev)
    student = KD._default_student(512, 8078673, 10, 4, 2).to(dev)
    params = student.multi_network.packed()
    m, v = torch.zeros_like(params), torch.zeros_like(params)
    ex = KD.distill_examples(dmin, dmax, 128, 0, 0)
    with torch.no_grad():
        traw = teacher({'pts': ex[..., :3].reshape(-1, 3), 'viewdirs': ex[..., 3:6].reshape(-1, 3)})['raw'].reshape(512, 128, 4)
    it = [0]

    def gen():
        it[0] += 1
        KD.distill_examples(dmin, dmax, 128, 0, it[0], out=ex)

    def query():
        with torch.no_grad():
            teacher({'pts': ex[..., :3].reshape(-1, 3), 'viewdirs': ex[..., 3:6].reshape(-1, 3)})

    adam = dict(m=m, v=v, step=1, lr=1e-3)
    loss = torch.empty(512, device=dev)

    def step():
        KD.student_step(ex, traw, dmin, dmax, params, 10, 4, 2, 0.0211, loss=loss, adam=adam)
    mn = student.multi_network
    opt = torch.optim.Adam(mn.parameters(), lr=1e-3)

    def bmm_step():
        opt.zero_grad()
        bmm_reference(bmm_params(mn), ex, traw, dmin, dmax).backward()
        opt.step()
    out = {'networks': 512, 'batch': 128}
    out['examples_us'] = timed(gen, args.iters)
    out['teacher_query_us'] = timed(query, max(5, args.iters // 5))
    out['student_step_us'] = timed(step, args.iters)
    out['bmm_step_us'] = timed(bmm_step, max(5, args.iters // 5))
    out['student_step_vs_teacher'] = out['student_step_us'] / out['teacher_query_us']
    out['bmm_over_fused'] = out['bmm_step_us'] / out['student_step_us']
    if not args.skip_occupancy:
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        occ = KD.build_occupancy_grid(teacher, gmin, gmax, [144, 256, 160])
        b.record()
        torch.cuda.synchronize()
        out['occupancy_ms'] = a.elapsed_time(b)
        out['occupancy_points'] = 144 * 256 * 160 * 27
        out['occupied_fraction'] = occ.float().mean().item()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
