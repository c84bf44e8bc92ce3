"""Golden fixture for the 3-D loader: batches of the reference's own ZeroDoseDataset3D + DataLoader (util.py:723-810) over synthetic volumes,
three shuffled epochs with aug and drop-off and one without aug.  Writes tests/golden/data3d_b2.npz; oracle/ is used as it is.

    python tools/gen_golden_data3d.py

The reference's source is imported while this runs and nowhere else.  Its class hard-codes 160 x 192 x 64 for the zero fill (`image_size` is set to
the fixture's size here) and loads a `BraTS_mean.npy` in its constructor (a throw-away one is made in a temporary working directory).
Per batch: subject ids, masks, inputs and targets in full as fp32, their float64 sums and the count of `== -10`; per epoch: the next
`np.random.rand()` after it, which pins the position of the global stream.  Same bytes on every run (fixed zip timestamps)."""
import io
import os
import sys
import tempfile
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)
from oracle import gen_golden as G                                           # noqa: E402
from fixtures_data3d import DATA3D_CFG, data3d_volumes, data3d_subjects      # noqa: E402


def save_npz(path, arrays):
    """np.savez_compressed with a fixed timestamp on every member"""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def record(out, tag, batch):
    x64 = batch['inputs'].numpy().astype(np.float64)
    x = x64.astype(np.float32)
    t = batch['targets'].numpy().astype(np.float32)
    out[f'subj_{tag}'] = np.array(batch['subj_id'])
    out[f'mask_{tag}'] = batch['mask'].numpy()
    out[f'slice_{tag}'] = batch['slice_idx'].numpy()
    out[f'insum_{tag}'] = np.array([x64.sum(), np.abs(x64).sum(), float((x64 == -10).sum())])
    out[f'tsum_{tag}'] = t.astype(np.float64).sum((1, 2, 3))
    out[f'inputs_{tag}'] = x
    out[f'targets_{tag}'] = t


def main():
    G.import_reference()
    import util as ref_util          # noqa
    from torch.utils.data import DataLoader
    c = DATA3D_CFG
    data = data3d_volumes()
    subj = np.array(data3d_subjects(data))
    Dz = c['D'] - 91
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            np.save('BraTS_mean.npy', np.zeros(1))
            mk = lambda aug: ref_util.ZeroDoseDataset3D('BraTS', data, subj, contrast_list=c['contrasts'], aug=aug, dropoff=True)
            ds_aug, ds_plain = mk(True), mk(False)
        finally:
            os.chdir(cwd)
    for ds in (ds_aug, ds_plain):
        ds.image_size = [c['H'], c['W'], Dz]
    np.random.seed(c['np_seed']); torch.manual_seed(c['torch_seed'])
    out, present, flips = {}, set(), 0
    for kind, ds, epochs in (('a', ds_aug, c['aug_epochs']), ('n', ds_plain, c['plain_epochs'])):
        for ep in range(epochs):
            for bi, batch in enumerate(DataLoader(ds, batch_size=c['batch_size'], shuffle=True, num_workers=0)):
                record(out, f'{kind}{ep}_{bi}', batch)
                present |= set(batch['mask'].sum(1).tolist())
            out[f'nbatch_{kind}{ep}'] = np.array(bi + 1)
            out[f'next_rand_{kind}{ep}'] = np.array(np.random.rand())        # one draw after every epoch: the tests make it too
    path = os.path.join(G.OUT, 'data3d_b2.npz')
    save_npz(path, out)
    print('data3d_b2:', sum(int(out[k]) for k in out if k.startswith('nbatch_')), 'batches; contrasts present per item', sorted(present),
          '; bytes', os.path.getsize(path))


if __name__ == '__main__':
    main()
