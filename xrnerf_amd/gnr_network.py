"""GNR's network (configs/gnr/gnr_genebody.py: model = GnrNetwork; the reference's networks/gnr.py): the image encoder
(gnr_encoder.HGFilter), optionally SRFilters, GNRMLP and GnrRenderer behind the reference's methods.  The encoder's output is a view
of a channel-last buffer, which the renderer's pixel gather reads as it is."""
import numpy as np
import torch
from torch import nn

from . import builder
from .builder import NETWORKS
from .gnr_render import index
from .networks import BaseNerfNetwork


def init_weights(net, init_gain=0.02):
    """networks/utils/gnr.py:27-63 with init_type='normal': N(0, init_gain) on every Conv / Linear weight, zero biases"""
    def init_func(m):
        name = m.__class__.__name__
        if hasattr(m, 'weight') and ('Conv' in name or 'Linear' in name):
            with torch.no_grad():
                m.weight.normal_(0.0, init_gain)
                if getattr(m, 'bias', None) is not None:
                    m.bias.zero_()
    net.apply(init_func)


@NETWORKS.register_module()
class GnrNetwork(BaseNerfNetwork):
    def __init__(self, cfg):
        super().__init__()
        self.name = 'gnr'
        self.cfg = cfg
        self.num_views = cfg.num_views
        self.use_feat_sr = cfg.use_feat_sr
        self.ddp = cfg.ddp
        self.feat_dim = 64 if self.use_feat_sr else 256
        self.index = index
        self.error_term = nn.MSELoss()
        self.metrics_dict = {'lpips': [], 'psnr': [], 'ssim': []}
        self.image_filter = builder.build_embedder(cfg.image_filter)
        if self.use_feat_sr:
            self.sr_filter = builder.build_embedder(cfg.sr_filter)
        if not cfg.train_encoder:
            for param in self.image_filter.parameters():
                param.requires_grad = False
        self.nerf = builder.build_mlp(cfg.nerf)
        cfg.nerf_renderer.opt.model = self.nerf
        self.nerf_renderer = builder.build_render(cfg.nerf_renderer)
        init_weights(self)

    def image_rescale(self, images, masks):
        if images.min() < -0.2:
            images = (images + 1) / 2
            images = images * (masks > 0).float()
        return images

    def get_image_feature(self, data):
        if 'feats' not in data.keys():
            images = data['images']
            im_feat = self.image_filter(images[:self.num_views])
            if self.use_feat_sr:
                im_feat = self.sr_filter(im_feat, images[:self.num_views])
            data['images'] = torch.cat([self.image_rescale(images[:self.num_views], data['masks'][:self.num_views]), images[self.num_views:]], 0)
            data['feats'] = im_feat
        return data

    def forward(self, data, is_test=False):
        data = self.get_image_feature(data)
        return self.nerf_renderer.render(**data)

    def render_path(self, data):
        with torch.no_grad():
            data = self.get_image_feature(data)
            rgbs, depths = self.nerf_renderer.render_path(**data)
        return rgbs, depths

    def reconstruct(self, data):
        """-> (verts float64 [Nv,3], faces int32 [T,3], rgbs float32 [Nv,3]): the textured body mesh of the frame"""
        if data.get('persps') is None:
            raise NotImplementedError('projection: only the perspective projection is built')
        with torch.no_grad():
            data = self.get_image_feature(data)
            return self.nerf_renderer.reconstruct(**data)

    def train_step(self, data, optimizer, **kwargs):
        return self.forward(self.prepare_data(self.cfg, data))

    def val_step(self, data, optimizer=None, **kwargs):
        test_data = data
        data = self.prepare_data(self.cfg, test_data)
        render_gt = test_data['render_gt'][0].to(data['images'].device)
        data_ren = self.get_image_feature(data)
        rgbs, depths = self.nerf_renderer.render_path(**data_ren)
        att_rgbs = rgbs[..., 3:6] if self.cfg.use_attention else rgbs[..., :3]
        re_att_rgbs = np.array([att_rgb for att_rgb in att_rgbs.cpu().numpy()])
        re_render_gt = np.array([gt for gt in render_gt.permute(0, 2, 3, 1).cpu().numpy()])
        return {'rgbs': re_att_rgbs, 'disps': depths.cpu(), 'rgb': re_att_rgbs, 'gt_img': re_render_gt, 'gt_imgs': re_render_gt,
                'idx': int(test_data['idx'].cpu())}

    def cal_metrics(self, metrics, rgbs, gts):
        x = rgbs.clone().permute((0, 3, 1, 2))
        out = {}
        for m_key in metrics.keys():
            out[m_key] = torch.stack([metrics[m_key](pred, gt) for pred, gt in zip(x, gts)], dim=0)
        return out

    def prepare_data(self, opt, data, local_rank=0):
        """the loader's batch (every entry behind a batch dimension of 1) -> the renderer's arguments, on device `local_rank` (the
        host when there is no device)"""
        dev = local_rank if torch.cuda.is_available() else 'cpu'
        smpl = None
        if any([opt.use_smpl_sdf, opt.use_t_pose]):
            smpl = {'rot': data['smpl_rot'].to(device=dev), 'verts': data['smpl_verts'][0].to(device=dev),
                    'faces': data['smpl_faces'][0].to(device=dev)}
            if opt.use_t_pose:
                smpl['t_verts'] = data['smpl_t_verts'][0].to(device=dev)
                smpl['t_faces'] = data['smpl_t_faces'][0].to(device=dev)
            if opt.use_smpl_depth:
                given = data.get('smpl_depth')
                if given is not None and len(given) > 0 and given[0].numel() > 0:
                    smpl['depth'] = given[0].to(device=dev)[:, None, ...]
                else:
                    # a frame without depth files (a re-posed body, a user's capture): the maps are rasterised from the body itself
                    from .gnr_raster import depth_maps
                    if opt.projection_mode != 'perspective':
                        raise NotImplementedError('projection: only the perspective projection is built')
                    r = self.nerf_renderer
                    smpl['depth'] = depth_maps(smpl['verts'], smpl['faces'], data['calib'][0].to(device=dev)[:self.num_views],
                                               data['persps'][0].to(device=dev)[:self.num_views], r.height, r.width)
        scan = [data['scan_verts'][0].to(device=dev), data['scan_faces'][0].to(device=dev)] if 'scan_verts' in data.keys() else None
        return {'images': data['img'][0].to(device=dev), 'calibs': data['calib'][0].to(device=dev),
                'bbox': list(data['bbox'][0].cpu().numpy().astype(np.int32)), 'masks': data['mask'][0].to(device=dev),
                'mesh_param': {'center': data['center'][0].to(device=dev), 'spatial_freq': data['spatial_freq'][0].cpu().numpy().item()},
                'smpl': smpl, 'scan': scan, 'persps': data['persps'][0].to(device=dev) if opt.projection_mode == 'perspective' else None}

    def to8b(self, img):
        if isinstance(img, torch.Tensor):
            img = img.detach().cpu().numpy()
        if img.shape[0] == 3 and img.shape[-1] != 3:
            img = np.transpose(img, [1, 2, 0])
        if img.min() < -.2:
            img = (img + 1) * 127.5
        elif img.max() <= 2.:
            img = img * 255.
        return np.clip(img, 0, 255).astype(np.uint8)
