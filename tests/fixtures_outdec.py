"""Seeded inputs of the output-decoder goldens (tools/gen_golden_outdec.py) that tests/fixtures.py does not have: the float targets of a
non-BraTS dataset, whose recon-y loss is the p-norm against an image (main_missing.py:195)."""
import torch

DECODERS = ('U', 'U+SA', 'U+SA+CA', 'U+SSA+CA')           # target_model_name, model.py:2955-2964
FUSE_METHODS = ('mean', 'max', 'mean-max-min')            # config.yaml:79


def make_float_targets(B, H, W, seed, ch=1):
    """(B, ch, H, W) non-negative float targets (a PET-like intensity map): the softplus decoder output is compared against them"""
    g = torch.Generator().manual_seed(seed)
    return 2.0 * torch.rand(B, ch, H, W, generator=g)
