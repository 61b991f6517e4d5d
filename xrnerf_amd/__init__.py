"""xrnerf_amd: MI355X-native Instant-NGP hot path behind openxrlab/xrnerf's module registry.

Importing the package registers the reference's type names (`HashNerfNetwork`, `NGPGridSampler`,
`HashNerfMLP`, `HashNerfRender`) in `xrnerf_amd.builder.MODELS`, so
`build_network(cfg.model)` works on the reference's configs/instant_ngp/*.py unchanged; likewise the
vanilla-NeRF (config #1, `vanilla.py`), Mip-NeRF (config #3, `mip.py`) and KiloNeRF (config #5, `kilo.py`; its distillation phase:
`kilo_distill.py`, run as the reference runs it by `kilo_tree.py`) BungeeNeRF (`bungee.py`), Animatable-NeRF (`aninerf.py`) NeuralBody (`neuralbody.py`) and GNR (`gnr.py`, `gnr_render.py`, `gnr_encoder.py`,
`gnr_network.py`; mesh reconstruction: `gnr_recon.py`) type names.  A reference config file trains and tests end to end through
`xrnerf_amd.apis` (`train_nerf`, `test_nerf`, `run_nerf`; `python -m xrnerf_amd.run_nerf`) on the runners of `xrnerf_amd.runner`.
"""
from . import builder  # noqa: F401
from .builder import build_embedder, build_mlp, build_network, build_render, build_sampler  # noqa: F401
from . import mlps, networks, renders, samplers, vanilla, mip, kilo, kilo_distill, kilo_tree, bungee, aninerf, neuralbody, gnr, gnr_render, gnr_encoder, gnr_network  # noqa: F401,E402

__version__ = '0.1.0'
