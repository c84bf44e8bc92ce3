"""Seeded inputs shared by tools/gen_golden_data3d.py and the data3d tests (tests/golden/data3d_b2.npz)."""
import numpy as np

from oracle.ref_data import synthetic_volumes

# five subjects, four contrasts, every third (subject + contrast) missing; D = 99 leaves Dz = 8 inside the reference's crop [45:-46]
DATA3D_CFG = dict(n_subj=5, contrasts=['T1', 'T1c', 'T2', 'T2_FLAIR'], H=16, W=24, D=99, seed=3, missing_every=3, batch_size=2,
                  np_seed=5, torch_seed=7, aug_epochs=3, plain_epochs=1)


def data3d_volumes(cfg=DATA3D_CFG, n_subj=None, H=None, W=None, D=None, contrasts=None, seed=None):
    """oracle.ref_data.synthetic_volumes with the zeros outside the ellipse set to -10 (the z-score files' background convention), so that the
    augmentation's `inputs[inputs == inputs.min()] = -10` has something to select.  Label volumes keep their zeros."""
    data = synthetic_volumes(n_subj or cfg['n_subj'], contrasts or cfg['contrasts'], H or cfg['H'], W or cfg['W'], D or cfg['D'],
                             cfg['seed'] if seed is None else seed, missing_every=cfg['missing_every'])
    for k, v in data.items():
        if not k.endswith('/seg'):
            v[v == 0] = -10.0
    return data


def data3d_subjects(data):
    return sorted({k.split('/')[0] for k in data})


def compose_item(data, subj_id, contrasts, drop, flip, scale, shift, aug, z0, Dz):
    """the item the 3-D loader stands for, in fp32 numpy: crop, zeros for absent / dropped contrasts, H flip, x * scale + shift with fp32-rounded
    parameters, -10 where the RAW value equals the item's raw minimum (csrc/mrdis_volgather.hip).  -> inputs (M, H, W, Dz), raw, targets (H, W, Dz)"""
    some = next(iter(data.values()))
    H, W = some.shape[:2]
    vols = [data.get(subj_id + '/' + c) if m != drop else None for m, c in enumerate(contrasts)]
    raw = np.stack([v[:, :, z0:z0 + Dz] if v is not None else np.zeros((H, W, Dz), np.float32) for v in vols]).astype(np.float32)
    seg = data.get(subj_id + '/seg')
    tgt = np.zeros((H, W, Dz), np.float32) if seg is None else seg[:, :, z0:z0 + Dz].astype(np.float32)
    tgt = np.where(tgt == 4, np.float32(3), tgt)
    if flip:
        raw, tgt = raw[:, ::-1], tgt[::-1]
    if not aug:
        return raw.copy(), raw, tgt.copy()
    m0 = min([v[:, :, z0:z0 + Dz].min() for v in vols if v is not None] + ([0.0] if any(v is None for v in vols) else []))
    x = raw * np.float32(scale) + np.float32(shift)
    x[raw == np.float32(m0)] = -10
    return x, raw, tgt.copy()


def aug_bound(raw, scale, shift):
    """|fp32 x * scale + shift - the reference's float64| <= 4 * 2^-24 * (|x| scale + |shift|): two roundings of the arithmetic plus the two
    parameter roundings, half an ulp each"""
    return 4 * 2.0 ** -24 * (np.abs(raw).astype(np.float64) * float(scale) + abs(float(shift)))
