"""Generates tests/golden/ref_vanilla_train.npz from the REFERENCE ITSELF (build container only): ONE TRAINING STEP of vanilla NeRF
(BASELINE config #1, small widths) through the reference's own NerfMLP / NerfRender / sample_pdf, imported with tests/golden/ref_import.py:
values of both passes, the loss, dL/draw of both passes and every parameter gradient -- plus a second render case with
raw_noise_std = 1.  Everything random is STORED: the draws are made by reseeding torch.manual_seed(7) and replaying the reference's
rand / randn calls in its call order (the live test tests/test_vanilla_nerf.py seeds the same way).

Run:  python tests/golden/make_golden_vanilla_train.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
MCFG = dict(skips=[2], netdepth=4, netwidth=32, output_ch=5, use_viewdirs=True, netchunk=1024 * 32,
            embedder=dict(type='BaseEmbedder', i_embed=0, multires=10, multires_dirs=4))
N_RAYS, N_COARSE, N_FINE, SEED = 48, 16, 24, 7


def main():
    import ref_import
    R = ref_import.load()
    torch.manual_seed(11)
    mlp, fine = R.NerfMLP(**MCFG), R.NerfMLP(**MCFG)
    render = R.NerfRender(white_bkgd=True, raw_noise_std=0)
    g = torch.Generator().manual_seed(5)
    rays_o = torch.randn(N_RAYS, 3, generator=g) * 0.1 + torch.tensor([0., 0., 4.])
    rays_d = torch.nn.functional.normalize(torch.randn(N_RAYS, 3, generator=g) * 0.2 - torch.tensor([0., 0., 1.]), dim=-1) * 1.3
    viewdirs = rays_d / rays_d.norm(dim=-1, keepdim=True)
    t = torch.linspace(0., 1., N_COARSE)
    z = (2. * (1 - t) + 6. * t).expand(N_RAYS, N_COARSE)
    mids = .5 * (z[..., 1:] + z[..., :-1])
    lower, upper = torch.cat([z[..., :1], mids], -1), torch.cat([mids, z[..., -1:]], -1)
    z = lower + (upper - lower) * torch.rand(N_RAYS, N_COARSE, generator=g)
    target = torch.rand(N_RAYS, 3, generator=g)
    # a density the small random MLP would not produce: shift the density bias so that some rays saturate
    with torch.no_grad():
        mlp.alpha_linear.bias.add_(0.5)
        fine.alpha_linear.bias.add_(0.5)
    out = dict(rays_o=rays_o.numpy(), rays_d=rays_d.numpy(), viewdirs=viewdirs.numpy(), z_vals=z.numpy(), target=target.numpy())
    for name, m in (('sd_coarse.', mlp), ('sd_fine.', fine)):
        for k, v in m.state_dict().items():
            out[name + k] = v.numpy().copy()

    # ---- one training step (nerf.py:71-92): coarse pass, perturbed resampling, fine pass, loss = mse(fine) + mse(coarse)
    torch.manual_seed(SEED)
    state = torch.random.get_rng_state()
    out['u'] = torch.rand(N_RAYS, N_FINE).numpy()                           # the one draw of the step: sample_pdf's torch.rand
    torch.random.set_rng_state(state)
    pts = rays_o[..., None, :] + rays_d[..., None, :] * z[..., :, None]
    data = {'pts': pts, 'viewdirs': viewdirs, 'z_vals': z, 'rays_o': rays_o, 'rays_d': rays_d}
    data = mlp(data)
    raw_c = data['raw']
    raw_c.retain_grad()
    data, ret = render(data, False)
    out['coarse_raw'], out['coarse_weights'] = raw_c.detach().numpy().copy(), data['weights'].detach().numpy().copy()
    for k in ('rgb', 'disp', 'acc'):
        out['coarse_' + k] = ret[k].detach().numpy().copy()
    seen = []
    sort = torch.sort

    def spy(x, *a, **k):
        seen.append(x.detach().clone())
        return sort(x, *a, **k)
    torch.sort = spy
    try:
        data = R.sample_pdf(data, N_FINE, True, False)
    finally:
        torch.sort = sort
    out['z_samples'] = seen[0][..., N_COARSE:].numpy().copy()              # the new samples before the merge
    out['fine_z'] = data['z_vals'].detach().numpy().copy()
    data = fine(data)
    raw_f = data['raw']
    raw_f.retain_grad()
    data, fret = render(data, False)
    out['fine_raw'], out['fine_weights'] = raw_f.detach().numpy().copy(), data['weights'].detach().numpy().copy()
    for k in ('rgb', 'disp', 'acc'):
        out['fine_' + k] = fret[k].detach().numpy().copy()
    loss = torch.mean((fret['rgb'] - target) ** 2) + torch.mean((ret['rgb'] - target) ** 2)
    loss.backward()
    out['loss'] = np.array([float(loss.detach())], np.float64)
    out['d_coarse_raw'], out['d_fine_raw'] = raw_c.grad.numpy().copy(), raw_f.grad.numpy().copy()
    for name, m in (('grad_coarse.', mlp), ('grad_fine.', fine)):
        for k, p in m.named_parameters():
            out[name + k] = p.grad.numpy().copy()

    # ---- second render case: raw_noise_std = 1 on the coarse raw (the reference draws randn(raw[..., 3].shape) * std)
    noisy = R.NerfRender(white_bkgd=True, raw_noise_std=1.0)
    torch.manual_seed(SEED)
    state = torch.random.get_rng_state()
    out['noise'] = (torch.randn(N_RAYS, N_COARSE) * 1.0).numpy()
    torch.random.set_rng_state(state)
    raw_n = torch.tensor(out['coarse_raw'], requires_grad=True)
    d2, r2 = noisy({'raw': raw_n, 'z_vals': z, 'rays_d': rays_d}, False)
    gr = torch.Generator().manual_seed(6)
    g_rgb = torch.randn(N_RAYS, 3, generator=gr)
    (r2['rgb'] * g_rgb).sum().backward()
    out['noisy_g_rgb'] = g_rgb.numpy()
    out['noisy_weights'], out['noisy_d_raw'] = d2['weights'].detach().numpy().copy(), raw_n.grad.numpy().copy()
    for k in ('rgb', 'disp', 'acc'):
        out['noisy_' + k] = r2[k].detach().numpy().copy()
    path = os.path.join(HERE, 'ref_vanilla_train.npz')
    np.savez_compressed(path, **out)
    print('ref_vanilla_train.npz', os.path.getsize(path) // 1024, 'KiB')


if __name__ == '__main__':
    main()
