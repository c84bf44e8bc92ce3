"""The label rule of the whole-subject 2-D segmentation (segment.py, csrc/mrdis_seg2d.hip) restated in numpy float64: the oracle of
tests/test_seg2d_cpu.py and tests/test_gpu_seg2d.py.  The rule is this package's own convention (the reference assembles no volume).

One view: argmax over the logits, the lowest class on a tie -- exact, no tolerance.  Two views: argmax of p = 0.5 (softmax(y^0) + softmax(y^1)),
view v read at the pixel mirrored per its flip code.  There a kernel in fp32 may legitimately pick another class where the two largest p are
closer than its rounding, so the oracle EXCLUDES a voxel from the label comparison iff the float64 top-two gap of p is below TAU = 1e-5.  A plain
fp32 evaluation of the rule was measured on the CPU at max |p32 - p64| = 1.4e-7, so TAU is about 70 times the rounding it must absorb; the excluded
share of a case is capped at CAP = 0.1 % of its voxels.  The cases use logits 3 * randn: small-scale logits (0.05 * randn) put 0.18 % of the voxels
inside TAU and break the cap."""
import numpy as np
import torch

TAU = 1e-5
CAP = 1e-3
FLIP_AXIS = {0: None, 1: 2, 2: 3}             # flip code -> axis of a (B, C, H, W) array

# the two-view cases of both test files: (name, flips, seed) at the base shape
BASE = dict(B=5, C=4, H=33, W=37, D=13)
TWO_VIEW_CASES = (('h', (0, 1), 101), ('w', (0, 2), 102), ('none', (0, 0), 103))


def make_logits(seed, B, C, H, W, scale=3.0):
    """fp32 (B, C, H, W) CPU tensor, scale * randn, from a seeded generator"""
    g = torch.Generator().manual_seed(seed)
    return scale * torch.randn(B, C, H, W, generator=g)


def unflip(y, code):
    ax = FLIP_AXIS[int(code)]
    return y if ax is None else np.flip(y, axis=ax)


def relabel_classes(lab, relabel):
    lab = lab.astype(np.uint8)
    if relabel:
        lab[lab == 3] = 4
    return lab


def labels_one_view(y, flip=0, relabel=False):
    """(B, H, W) uint8: argmax over the channels of the logits themselves (np.argmax returns the first maximum: the lowest class on a tie)"""
    y = unflip(np.asarray(y, dtype=np.float64), flip)
    return relabel_classes(np.argmax(y, axis=1), relabel)


def softmax(y, dtype):
    y = np.asarray(y, dtype=dtype)
    e = np.exp(y - y.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def probs_two_views(views, flips, dtype=np.float64):
    a, b = (softmax(unflip(np.asarray(v), f), dtype) for v, f in zip(views, flips))
    return dtype(0.5) * (a + b)


def labels_two_views(views, flips, relabel=False):
    """-> (labels (B, H, W) uint8, excluded (B, H, W) bool: the float64 top-two gap of p is below TAU)"""
    p = probs_two_views(views, flips, np.float64)
    top = np.sort(p, axis=1)
    excluded = (top[:, -1] - top[:, -2]) < TAU
    return relabel_classes(np.argmax(p, axis=1), relabel), excluded


def labels_two_views_fp32(views, flips, relabel=False):
    """the rule evaluated plainly in fp32 with torch on the CPU: the stand-in for the kernel in the CPU test -> (labels, p32)"""
    ps = []
    for v, f in zip(views, flips):
        y = torch.as_tensor(np.ascontiguousarray(unflip(np.asarray(v, dtype=np.float32), f)))
        e = torch.exp(y - y.max(dim=1, keepdim=True).values)
        ps.append(e / e.sum(dim=1, keepdim=True))
    p = 0.5 * (ps[0] + ps[1])
    return relabel_classes(torch.argmax(p, dim=1).numpy(), relabel), p.numpy()


def place(planes, labels, s0):
    """planes (D, H, W) uint8, labels (B, H, W): the planes s0 .. s0 + B - 1 become the labels, in place"""
    planes[s0:s0 + labels.shape[0]] = labels
    return planes


def two_view_inputs(seed):
    s = BASE
    return [make_logits(seed, s['B'], s['C'], s['H'], s['W']).numpy(), make_logits(seed + 1000, s['B'], s['C'], s['H'], s['W']).numpy()]
