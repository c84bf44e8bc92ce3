"""Golden fixture for the segmentation metrics: the reference's own `compute_segmentation_metrics` (util.py:946-992) on a small seeded case.
Writes tests/golden/segmetrics3d.npz (inputs and outputs); oracle/ is used as it is.

    python tools/gen_golden_seg3d.py

The reference's source is imported while this runs and nowhere else.  The case: B = 3 label volumes of 8^3 with labels 0..3 and 3-channel
fp32 predictions; sample 1 has no voxel of class 3, sample 0 carries predictions equal to exactly 0.5 (not above the threshold) on labelled and
unlabelled voxels, sample 2's prediction is empty (nothing above 0.5).  Same bytes on every run (fixed zip timestamps)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)
from oracle import gen_golden as G                                           # noqa: E402
from gen_golden_data3d import save_npz                                        # noqa: E402

SEED, B, S = 17, 3, 8


def case():
    g = np.random.RandomState(SEED)
    labels = g.randint(0, 4, (B, S, S, S)).astype(np.float32)
    labels[1][labels[1] == 3] = 0                                            # a class absent from one sample
    pred = g.rand(B, 3, S, S, S).astype(np.float32)
    region = np.stack([(labels == c + 1) for c in range(3)], 1)
    pred = np.where(region, np.float32(0.35) + np.float32(0.6) * pred, np.float32(0.7) * pred).astype(np.float32)   # mostly right, some misses and false alarms
    pred[0, :, 0, :, :] = 0.5                                                # exactly at the threshold: not predicted
    pred[2] = np.float32(0.5) * pred[2]                                      # one empty prediction
    return labels, pred


def main():
    G.import_reference()
    import util as ref_util          # noqa
    labels, pred = case()
    assert (labels[1] == 3).sum() == 0 and (pred == 0.5).sum() > 0 and (pred[2] > 0.5).sum() == 0 and (pred[0] > 0.5).sum() > 0
    m = ref_util.compute_segmentation_metrics(labels, pred)
    out = {'labels': labels, 'pred': pred, 'dice': np.array(m['dice'], dtype=np.float64), 'iou': np.array(m['iou'], dtype=np.float64)}
    path = os.path.join(G.OUT, 'segmetrics3d.npz')
    save_npz(path, out)
    print('segmetrics3d: dice', out['dice'], 'iou', out['iou'], '; bytes', os.path.getsize(path))


if __name__ == '__main__':
    main()
