"""xrnerf_amd/bungeedata.py and xrnerf_amd/kilodata.py without a GPU: the registries, the planners, the NSVF loader and the node
dataset's checkpoint against tests/golden/ref_scenedata.npz, the refusals that need no kernel, and the agreement of the header, the
ctypes table and the build recipe."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import scenedata_cases as K  # noqa: E402
from xrnerf_amd import bungeedata, kilodata  # noqa: E402,F401  (every check here is about these modules)


def test_header_table_and_build_recipe_agree():
    K.check_symbols(loaded=False)


def test_every_data_type_of_the_reference_configs_is_registered():
    K.check_registries()


def test_planners_take_the_config_lists_and_leave_the_existing_ones():
    K.check_plans()


def test_nsvf_loader_reproduces_the_fixture(tmp_path):
    K.check_nsvf_loader(str(tmp_path))


def test_node_dataset_checkpoint_and_boxes_are_the_fixture(tmp_path):
    K.check_node_cp(str(tmp_path))


def test_refusals(tmp_path):
    K.check_refusals_host(str(tmp_path))


def test_restatement_rounds_to_the_fixture():
    """the float64 lines of tests/scenedata_restatement.py, rounded to fp32 once, are the fixture's training rays (stage 1)"""
    import numpy as np
    import scenedata_restatement as RS
    g, c = K.gold(), K.city()
    poses, images = c['poses'][2:], np.clip(np.rint(c['images'][2:] * 255.), 0, 255).astype(np.uint8).astype(np.float32) / 255
    spec = RS.table(K.H, K.W, np.float64(c['focal']), poses, images, bungeedata.scale_codes(4, 6, c['scale_split'], 1), g['bungee.s1.i_train'], g['bungee.s1.perm'])
    for k in K.RAY_KEYS:
        K.same_bits(spec[k] if k == 'scale_code' else spec[k].astype(np.float32), g['bungee.s1.' + k], 'restatement ' + k)
