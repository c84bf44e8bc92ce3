"""Batch assembly of the reference's volume dataset (`src/util.py:723-843`: ZeroDoseDataset3D, ZeroDoseDataAll3D) with the volumes resident in HBM.

The reference builds an item on the host -- an h5 read per contrast, `np.stack`, a flip made by subtracting a zeros array, a float64
scale/shift pass and an `== min()` pass -- and its training loop would then copy 31 MB per sample (4 x 160 x 192 x 64 fp32) to the GPU.
Here the volumes are uploaded once, as the h5 file has them ((H, W, D), D fastest), and a batch is ONE gather launch for the inputs and one for
the targets (`mrdis_volume_gather`, csrc/mrdis_volgather.hip), both driven by one small per-batch table, writing the channels-last-3d layout
the Conv3d kernels of model3d read.

Host-side behaviour follows the reference statement by statement:
  * depth crop `[:, :, 45:-46]` (`45:-47` for 'ZeroDose'): z0 = 45, Dz = D - 91 (D - 92)                         util.py:766-769
  * a contrast missing for a subject gives zeros and mask 0                                                      util.py:771-773
  * targets: '/PET' (ZeroDose), '/seg' with label 4 -> 3 (BraTS), zeros otherwise                                util.py:777-789
  * drop-off: `np.random.rand() > 0.8` then `np.random.choice(present, 1)`, only with dropoff and > 1 present      util.py:791-795
  * aug: `rand() > 0.5` flips H (inputs and targets), `1 + 0.2 (rand() - 0.5)` scales, `0.2 (rand() - 0.5)` shifts,
    then `inputs[inputs == inputs.min()] = -10` -- same global-RNG call order                                    util.py:798-805
  * slice_idx = 0                                                                                                util.py:807
  * batch order: `DataLoader(shuffle)`, reproduced draw for draw by BatchLoader._order.

Patch training (`patch_size`; THIS PACKAGE'S CONVENTION, the reference has none; off by default, and then nothing below runs): a training item is
a random (PH, PW, PD) sub-volume of the WHOLE stored scan instead of the depth crop, a share `patch_fg` of the items centred on a voxel of a
tumour class the subject has (csrc/mrdis_patch.hip, patch3d.py).  Per item the host draws, from the stream `meta` uses anyway and in this order:
  1. the reference's drop-off draws, unchanged
  2. `fg = rand() < patch_fg`, only if patch_fg > 0
  3. five uint32 `u_class, u_voxel, u_h, u_w, u_d` by one `randint(0, 2**32, size=5, dtype=np.uint32)`
  4. with aug: one `rand() > 0.5` per axis named in `patch_flips`, in h, w, d order
  5. with aug: scale and shift, as above
With `patch_warp` > 0 (and aug) a step 4b follows the flips: one `r = rand(5)` per item, always drawn -- `warp = r[0] < patch_warp`,
`angle_a = (2 r[1 + a] - 1) patch_rot[a]` degrees about the H, W, D axes, `zoom = lo + r[4] (hi - lo)` over `patch_zoom` -- and the batch is
gathered by patch3d.patch_warp (csrc/mrdis_warp.hip: integer coordinates, exact labels) instead of patch_gather.  With `patch_warp` = 0
no draw is added and every stream, batch and checkpoint is what it was.
With any of `patch_blur`, `patch_contrast`, `patch_gamma`, `patch_noise` > 0 (and aug) a step 4c follows the warp draw (or the flips), before scale
and shift, always in full: `r = rand(4 + 6 M)` and the noise seed `randint(0, 2**32, size=2, dtype=np.uint32)`.  The item coins are
`r[0] < patch_blur`, `r[1] < patch_contrast`, `r[2] < patch_gamma`, `r[3] < patch_noise`; per contrast m, q = r[4 + 6 m:10 + 6 m]: blurred iff
the blur coin and `q[0] < 0.5`, `sigma = lo + q[1] (hi - lo)`, the contrast factor, the gamma exponent and the noise deviation likewise from
q[2], q[3], q[5] over their ranges, and the inverted gamma curve iff `q[4] < patch_gamma_invert`; every value rounded once to fp32; an absent or
dropped contrast gets no flag.  The gathered inputs then pass through tone3d.patch_intensify (csrc/mrdis_tone.hip).  With the four shares at 0
no draw is added and no kernel launches.
The device turns the draws into the patch origin turns the draws into the patch origin (patch3d's docstring: pick, clamping instead of padding).  The `== min()` rule compares
with the minimum of the whole stored volume.  The evaluation loaders serve the centre patch, without a draw; `crop()` is then the centre
depth window of the trained depth PD, so the windowed reads slide PD over the full H x W.
The commented-out mean-image imputation (`img_mean`, `BraTS_mean.npy`) and the `missing` argument the reference never reads are not built.
"""
import os

import numpy as np
import torch

from . import hip, patch3d, tone3d
from .data import VolumeStore, BatchLoader

Z0 = 45                     # util.py:766-769


class VolumeStore3D(VolumeStore):
    """`data[subject + '/' + contrast]` of the reference's h5 file, kept on the device in the file's own layout (H, W, D): the depth crop of one
    (h, w) column is then one contiguous run, which is what the gather kernel reads.  Also keeps every volume's minimum inside a depth crop
    (the `== min()` rule of the augmentation needs it, csrc/mrdis_volgather.hip), computed on the device when a loader first asks."""

    def __init__(self, device):
        super().__init__(device)
        self._mins = {}             # (z0, Dz) -> (fp32 device tensor, {key: row})
        self._prefix = {}           # (key, classes) -> int32 device tensor (nblk + 1, K): patch3d.fg_prefix of a label volume

    def add(self, key, array_hwd):
        """key = 'subject/contrast' (h5 path); array in the reference layout (H, W, D)."""
        a = torch.as_tensor(np.ascontiguousarray(array_hwd), dtype=torch.float32)
        if a.dim() != 3:
            raise ValueError('volume must be (H, W, D)')
        if self.shape is None:
            self.shape = tuple(a.shape)
        elif tuple(a.shape) != self.shape:
            raise ValueError(f'{key}: shape {tuple(a.shape)} != {self.shape}')
        self.vols[key] = a.to(self.device)
        self._mins.clear()
        self._prefix.clear()

    def add_device(self, key, vol_hwd):
        """key = 'subject/contrast'; an fp32 device tensor already laid out as the store keeps it, (H, W, D) (prep.prep_write layout 'hwd'): kept as it is."""
        self._check_device_volume(key, vol_hwd, tuple(vol_hwd.shape) if getattr(vol_hwd, 'ndim', 0) == 3 else ())
        self.vols[key] = vol_hwd
        self._mins.clear()
        self._prefix.clear()

    def crop_min_ptr(self, key, z0, Dz):
        """device address of min(vol[:, :, z0:z0+Dz]) (fp32), 0 for a key the store does not hold.  No host read, no sync."""
        ent = self._mins.get((z0, Dz))
        if ent is None:
            keys = list(self.vols)
            mins = torch.stack([self.vols[k][:, :, z0:z0 + Dz].amin() for k in keys]) if keys else torch.empty(0, device=self.device)
            ent = self._mins[(z0, Dz)] = (mins.contiguous(), {k: i for i, k in enumerate(keys)})
        mins, rows = ent
        i = rows.get(key)
        return 0 if i is None else mins.data_ptr() + 4 * i

    def fg_prefix_ptr(self, key, classes):
        """device address of the label volume's prefix table over `classes` (patch3d.fg_prefix: one kernel launch and a running sum, once per
        volume, when a loader first asks), 0 for a key the store does not hold.  No host read, no sync."""
        v = self.vols.get(key)
        if v is None:
            return 0
        ent = self._prefix.get((key, classes))
        if ent is None:
            ent = self._prefix[(key, classes)] = patch3d.fg_prefix(v, classes)
        return ent.data_ptr()


def load_subj_list(path):
    """util.py:841-843: one subject id per line.  The reference reads the file with `pd.read_csv(path, sep=" ")` WITHOUT `header=None`, so pandas takes
    the first line as a header and the first subject of every list is never served; kept, since the reference's folds were run that way."""
    import pandas as pd
    lines = pd.read_csv(path, sep=' ')
    return np.array(lines.iloc[:, 0])


def patch_args(patch_size, patch_fg=0.0, patch_flips='h'):
    """-> ((PH, PW, PD) or None, patch_fg, patch_flips) checked: three integers >= 1, a share in 0 .. 1, distinct axes of 'hwd'; else ValueError"""
    if patch_size is not None:
        try:
            ok = len(patch_size) == 3 and all(not isinstance(v, bool) and int(v) == v and v >= 1 for v in patch_size)
        except TypeError:
            ok = False
        if not ok:
            raise ValueError(f'patch_size {patch_size!r}: None or three integers >= 1 (PH, PW, PD)')
        patch_size = tuple(int(v) for v in patch_size)
    if isinstance(patch_fg, bool) or not isinstance(patch_fg, (int, float)) or not 0.0 <= patch_fg <= 1.0:
        raise ValueError(f'patch_fg {patch_fg!r}: the share of foreground patches, 0 .. 1')
    if not isinstance(patch_flips, str) or any(a not in 'hwd' for a in patch_flips) or len(set(patch_flips)) != len(patch_flips):
        raise ValueError(f'patch_flips {patch_flips!r}: the axes that may flip, distinct letters of "hwd" (or the empty string)')
    return patch_size, float(patch_fg), patch_flips


def patch_warp_args(patch_warp=0.0, patch_rot=(30, 30, 30), patch_zoom=(0.7, 1.4)):
    """-> (patch_warp, (rot h, rot w, rot d), (zoom lo, zoom hi)) checked: a share in 0 .. 1, three largest absolute angles in 0 .. 45 degrees,
    lo <= hi both in 0.5 .. 2; else ValueError naming the key"""
    num = lambda v: not isinstance(v, bool) and isinstance(v, (int, float)) and np.isfinite(v)
    if not num(patch_warp) or not 0.0 <= patch_warp <= 1.0:
        raise ValueError(f'patch_warp {patch_warp!r}: the share of resampled training patches, 0 .. 1')
    try:
        ok = len(patch_rot) == 3 and all(num(v) and 0 <= v <= 45 for v in patch_rot)
    except TypeError:
        ok = False
    if not ok:
        raise ValueError(f'patch_rot {patch_rot!r}: the largest absolute rotation about the H, W and D axes, three numbers in 0 .. 45 degrees')
    try:
        ok = len(patch_zoom) == 2 and all(num(v) and 0.5 <= v <= 2 for v in patch_zoom) and patch_zoom[0] <= patch_zoom[1]
    except TypeError:
        ok = False
    if not ok:
        raise ValueError(f'patch_zoom {patch_zoom!r}: [lo, hi] with lo <= hi, both in 0.5 .. 2')
    return float(patch_warp), tuple(float(v) for v in patch_rot), tuple(float(v) for v in patch_zoom)


INTENSITY_DEFAULTS = {'patch_blur': 0.0, 'patch_blur_sigma': (0.5, 1.0), 'patch_contrast': 0.0, 'patch_contrast_range': (0.75, 1.25), 'patch_gamma': 0.0,
                      'patch_gamma_range': (0.7, 1.5), 'patch_gamma_invert': 0.25, 'patch_noise': 0.0, 'patch_noise_std': (0.0, 0.3)}
_INTENSITY_RANGES = {'patch_blur_sigma': (0.25, 1.0, 'sigma in voxels (the tap radius is 4)'), 'patch_contrast_range': (0.5, 2.0, 'the contrast factor'),
                     'patch_gamma_range': (0.5, 2.0, 'the gamma exponent'), 'patch_noise_std': (0.0, 1.0, 'the standard deviation of the noise, store units')}


def patch_intensity_args(**keys):
    """the nine intensity keys (INTENSITY_DEFAULTS for those not given) -> a dict of them, checked: the shares `patch_blur`, `patch_contrast`,
    `patch_gamma`, `patch_gamma_invert`, `patch_noise` in 0 .. 1; `patch_blur_sigma` [lo, hi] in 0.25 .. 1, `patch_contrast_range` and
    `patch_gamma_range` in 0.5 .. 2, `patch_noise_std` in 0 .. 1, each with lo <= hi; else ValueError naming the key (TypeError: no such key)"""
    unknown = sorted(set(keys) - set(INTENSITY_DEFAULTS))
    if unknown:
        raise TypeError(f'no intensity key {unknown}: one of {sorted(INTENSITY_DEFAULTS)}')
    num = lambda v: not isinstance(v, bool) and isinstance(v, (int, float)) and np.isfinite(v)
    out = {}
    for key, dflt in INTENSITY_DEFAULTS.items():
        v = keys.get(key, dflt)
        if key not in _INTENSITY_RANGES:
            if not num(v) or not 0.0 <= v <= 1.0:
                raise ValueError(f'{key} {v!r}: a share, 0 .. 1')
            out[key] = float(v)
            continue
        a, b, what = _INTENSITY_RANGES[key]
        try:
            ok = len(v) == 2 and all(num(e) and a <= e <= b for e in v) and v[0] <= v[1]
        except TypeError:
            ok = False
        if not ok:
            raise ValueError(f'{key} {v!r}: [lo, hi] of {what}, lo <= hi, both in {a} .. {b}')
        out[key] = (float(v[0]), float(v[1]))
    return out


class VolumeDataset3D:
    """ZeroDoseDataset3D (util.py:723-810) over a VolumeStore3D: `meta(idx)` is the host part of `__getitem__`.  `patch_size` (PH, PW, PD):
    patch training, see the module docstring; `patch_centre`: the deterministic centre patch instead of a random one (evaluation)."""

    TARGET_KEYS = {'ZeroDose': '/PET', 'BraTS': '/seg'}
    FG_CLASSES = {'BraTS': (1, 2, 4)}      # the label values a foreground patch may be centred on

    def __init__(self, dataset_name, store, subj_list, contrast_list=('T1',), aug=False, dropoff=False, patch_size=None, patch_fg=0.0,
                 patch_flips='h', patch_centre=False, patch_warp=0.0, patch_rot=(30, 30, 30), patch_zoom=(0.7, 1.4), **intensity):
        self.dataset_name, self.store = dataset_name, store
        self.subj_list, self.contrast_list = list(subj_list), list(contrast_list)
        self.aug, self.dropoff = aug, dropoff
        self.set_patch(patch_size, patch_fg, patch_flips, patch_centre, patch_warp, patch_rot, patch_zoom, **intensity)

    def set_patch(self, patch_size, patch_fg=0.0, patch_flips='h', patch_centre=False, patch_warp=0.0, patch_rot=(30, 30, 30), patch_zoom=(0.7, 1.4),
                  **intensity):
        """`intensity`: the keys of `patch_intensity_args` (patch_blur .. patch_noise_std), kept checked in `self.intensity`"""
        self.patch_size, self.patch_fg, self.patch_flips = patch_args(patch_size, patch_fg, patch_flips)
        self.patch_centre = bool(patch_centre)
        self.patch_warp, self.patch_rot, self.patch_zoom = patch_warp_args(patch_warp, patch_rot, patch_zoom)
        self.intensity = patch_intensity_args(**intensity)
        if self.patch_size is None:
            return
        if self.patch_fg > 0 and self.dataset_name not in self.FG_CLASSES:
            raise ValueError(f'patch_fg > 0 needs a dataset with label targets ({sorted(self.FG_CLASSES)}), not {self.dataset_name!r}')
        if self.store.shape is not None and any(p > n for p, n in zip(self.patch_size, self.store.shape)):
            raise ValueError(f'patch_size {self.patch_size} does not fit the stored volumes {tuple(self.store.shape)}: no padding past the border')

    def __len__(self):
        return len(self.subj_list)

    def crop(self):
        """(z0, Dz) of `[:, :, 45:-46]` (`45:-47` for 'ZeroDose'); in patch mode the centre depth window of the trained depth, ((D - PD) // 2, PD)."""
        if self.patch_size is not None:
            D, PD = self.store.shape[2], self.patch_size[2]
            if PD > D:
                raise ValueError(f'patch depth {PD} beyond the stored depth {D}')
            return (D - PD) // 2, PD
        Dz = self.store.shape[2] - Z0 - (47 if self.dataset_name == 'ZeroDose' else 46)
        if Dz < 1:
            raise ValueError(f'volumes of depth {self.store.shape[2]} leave nothing inside the crop')
        return Z0, Dz

    def meta(self, idx, rng=None, plain=False):
        """-> (subj_id, slice_idx = 0, volume pointers, dropped contrast or -1, target pointer, flip, scale, shift).  rng: None = the global np.random (the
        reference's own stream, draw for draw) or the loader's own np.random.RandomState (data-parallel runs, see BatchLoader).  `plain`: the item as
        stored -- nothing dropped, not augmented -- and no draw from any stream (the windowed reads of VolumeLoader3D.batches(z0=...)).
        In patch mode (and not `plain`) a ninth element follows: (fg, the five uint32 draws, (flip h, flip w, flip d), centre), and with
        `patch_warp` > 0 on an augmenting, non-centre dataset three more in it: (warp, (angle h, w, d) in degrees, zoom); where the dataset
        `intensifies()` one more after those: (seed (2,) uint32, flags (M,) of tone3d.BLUR | .., sigma, f, gamma, std, each (M,) float32)."""
        rng = np.random if rng is None else rng
        subj_id = str(self.subj_list[idx])
        ptrs = [self.store.ptr(subj_id + '/' + c) for c in self.contrast_list]
        mask = np.array([1 if p else 0 for p in ptrs])
        tkey = self.TARGET_KEYS.get(self.dataset_name)
        tptr = self.store.ptr(subj_id + tkey) if tkey else 0
        if plain:
            return subj_id, 0, ptrs, -1, tptr, False, 1.0, 0.0
        drop = -1
        if self.dropoff and mask.sum() > 1:                           # :791-795, same RNG call order
            if rng.rand() > 0.8:
                drop = int(rng.choice(np.where(mask == 1)[0], 1)[0])
        if self.patch_size is not None:
            return (subj_id, 0, ptrs, drop, tptr) + self._patch_draws(rng, [bool(p) and m != drop for m, p in enumerate(ptrs)])
        flip, scale, shift = False, 1.0, 0.0
        if self.aug:                                                  # :798-804
            flip = bool(rng.rand() > 0.5)
            scale = 1 + 0.2 * (rng.rand() - 0.5)
            shift = 0.2 * (rng.rand() - 0.5)
        return subj_id, 0, ptrs, drop, tptr, flip, scale, shift

    def _patch_draws(self, rng, present):
        """the tail of a patch-mode meta, drawn in the order of the module docstring: (flip h, scale, shift, (fg, u[5], flips, centre)), the last
        tuple followed by (warp, angles, zoom) where `warps()` and by the intensity draws where `intensifies()`.  present: per contrast, whether
        the item has it (and it is not dropped)"""
        if self.patch_centre:
            return False, 1.0, 0.0, (False, np.zeros(5, dtype=np.uint32), (False, False, False), True)
        fg = bool(rng.rand() < self.patch_fg) if self.patch_fg > 0 else False
        u = rng.randint(0, 2 ** 32, size=5, dtype=np.uint32)
        flips, scale, shift, warp, tone = [False, False, False], 1.0, 0.0, (), ()
        if self.aug:
            for i, axis in enumerate('hwd'):
                if axis in self.patch_flips:
                    flips[i] = bool(rng.rand() > 0.5)
            if self.patch_warp > 0:                                   # five doubles, always: the stream does not depend on the outcome
                r = rng.rand(5)
                lo, hi = self.patch_zoom
                warp = (bool(r[0] < self.patch_warp), tuple(float((2 * r[1 + a] - 1) * self.patch_rot[a]) for a in range(3)), float(lo + r[4] * (hi - lo)))
            if self.intensifies():                                    # 4 + 6 M doubles and the seed, always
                tone = (self._intensity_draws(rng, present),)
            scale = 1 + 0.2 * (rng.rand() - 0.5)
            shift = 0.2 * (rng.rand() - 0.5)
        return flips[0], scale, shift, (fg, u, tuple(flips), False) + warp + tone

    def _intensity_draws(self, rng, present):
        """step 4c of the module docstring -> (seed, flags, sigma, f, gamma, std)"""
        k, M = self.intensity, len(self.contrast_list)
        r = rng.rand(4 + 6 * M)
        seed = rng.randint(0, 2 ** 32, size=2, dtype=np.uint32)
        blur_on, contrast_on, gamma_on, noise_on = r[0] < k['patch_blur'], r[1] < k['patch_contrast'], r[2] < k['patch_gamma'], r[3] < k['patch_noise']
        q = r[4:].reshape(M, 6)
        span = lambda key, col: (k[key][0] + q[:, col] * (k[key][1] - k[key][0])).astype(np.float32)
        flags = []
        for m in range(M):
            f = 0
            if present[m]:
                f |= tone3d.BLUR if blur_on and q[m, 0] < 0.5 else 0
                f |= tone3d.CONTRAST if contrast_on else 0
                f |= (tone3d.GAMMA | (tone3d.INVERT if q[m, 4] < k['patch_gamma_invert'] else 0)) if gamma_on else 0
                f |= tone3d.NOISE if noise_on else 0
            flags.append(f)
        return seed, tuple(flags), span('patch_blur_sigma', 1), span('patch_contrast_range', 2), span('patch_gamma_range', 3), span('patch_noise_std', 5)

    def warps(self):
        """whether this dataset's batches go through patch3d.patch_warp: patch mode, augmenting, not the centre patch, patch_warp > 0"""
        return self.patch_size is not None and bool(self.aug) and not self.patch_centre and self.patch_warp > 0

    def intensifies(self):
        """whether this dataset's inputs go through tone3d.patch_intensify: patch mode, augmenting, not the centre patch, and any of patch_blur,
        patch_contrast, patch_gamma, patch_noise above 0"""
        return (self.patch_size is not None and bool(self.aug) and not self.patch_centre
                and any(self.intensity[key] > 0 for key in ('patch_blur', 'patch_contrast', 'patch_gamma', 'patch_noise')))

    def tone_col(self):
        """the word of a `patch_table` row at which the intensity block starts"""
        return 2 * len(self.contrast_list) + patch3d.TABLE_EXTRA + (patch3d.WARP_EXTRA if self.warps() else 0)


class VolumeLoader3D(BatchLoader):
    """DataLoader(dataset, batch_size, shuffle, num_workers=0) of util.py:837-839 over a VolumeDataset3D; yields the reference's sample dict with
    device tensors: inputs (B, M, H, W, Dz) channels-last-3d, targets (B, H, W, Dz) -- or, with `region_channels` = K, (B, K, H, W, Dz)
    channels-last-3d with channel c = (label == c + 1), this package's convention for `nvnet_loss` -- mask (B, M), subj_id (list), slice_idx (B,)
    zeros, plus mask_host and batch_index as in the 2-D loader.  The partial last batch is served.

    Batch order, rank / world / equal_steps and the loader's own stream under world > 1 are BatchLoader's (see its docstring); here that
    stream carries ALL per-item draws, drop-off and augmentation, for the same reason.

    `patch_size` (with `patch_fg`, `patch_flips`, `patch_centre`, `patch_warp`, `patch_rot`, `patch_zoom` and the intensity keys of
    `patch_intensity_args`; an intensifying loader adds three launches -- blur, statistics, tone -- on the inputs): puts the dataset into patch mode
    (VolumeDataset3D.set_patch; None leaves it as it was built).  A batch is then three launches -- origins, inputs, targets -- of (PH, PW, PD) patches, and carries 'origins' (B, 4) int32
    on the device: h0, w0, d0 and the index of the class a foreground patch was centred on (-1: uniform or centre)."""

    def __init__(self, dataset, batch_size, shuffle=False, rank=0, world=1, equal_steps=False, generator=None, region_channels=0,
                 patch_size=None, patch_fg=0.0, patch_flips='h', patch_centre=False, patch_warp=0.0, patch_rot=(30, 30, 30), patch_zoom=(0.7, 1.4),
                 **intensity):
        super().__init__(dataset, batch_size, shuffle, rank, world, equal_steps, generator)
        self.region_channels = int(region_channels)
        if patch_size is not None:
            dataset.set_patch(patch_size, patch_fg, patch_flips, patch_centre, patch_warp, patch_rot, patch_zoom, **intensity)
        else:
            patch_intensity_args(**intensity)                         # (read only with patch_size; a misspelt key is still an error)

    def _table_head(self, metas, width, crop, aug):
        """(B, width) int64 with the 2 M + 3 words every gather reads (include/mrdis.h mrdis_volume_gather) filled in and zeros beyond, and the
        host twin of `mask`.  `crop`: the (z0, Dz) whose minima the rows point to, None: no minima; the flag word gets the H flip and `aug`."""
        ds, st = self.dataset, self.dataset.store
        M = len(ds.contrast_list)
        tab = np.zeros((len(metas), width), dtype=np.int64)
        mask_host = np.zeros((len(metas), M), dtype=np.float32)        # host twin of `mask`: a loss may branch on it without a sync
        for r, (subj_id, _, ptrs, drop, tptr, flip, scale, shift, *_) in enumerate(metas):
            for m, p in enumerate(ptrs):
                if p and m != drop:
                    tab[r, m] = p
                    tab[r, M + m] = st.crop_min_ptr(subj_id + '/' + ds.contrast_list[m], *crop) if crop is not None else 0
                    mask_host[r, m] = 1.0
            tab[r, 2 * M] = tptr
            tab[r, 2 * M + 1] = (patch3d.FLIP_H if flip else 0) | (patch3d.AUG if aug else 0)
            bits = np.array([scale, shift], dtype=np.float32).view(np.uint32).astype(np.uint64)
            tab[r, 2 * M + 2] = (bits[0] | (bits[1] << np.uint64(32))).view(np.int64)
        return tab, mask_host

    def table(self, metas, plain=False):
        """the per-batch table of mrdis_volume_gather (include/mrdis.h), on the host, and the host twin of `mask`.  `plain`: the augment bit stays
        clear whatever the dataset says, and no crop minima are looked up (only the augmentation reads them; they belong to the crop's own z0)."""
        ds = self.dataset
        crop = ds.crop()
        return self._table_head(metas, 2 * len(ds.contrast_list) + 3, None if plain else crop, ds.aug and not plain)

    def patch_table(self, metas):
        """the per-batch table of mrdis_patch_origins / mrdis_patch_gather (include/mrdis.h: the words of `table`, the minima those of the whole
        volumes, then the prefix pointer, the flags and the packed draws), on the host, and the host twin of `mask`.  Where the dataset
        `warps()` the rows are patch3d.WARP_EXTRA words longer (mrdis_patch_warp): the WARP flag and the packed Q16 matrix of the items that drew
        a warp, zeros for the others.  Where it `intensifies()` they are tone3d.TONE_EXTRA(M) words longer still, from word `tone_col()`: the
        block of tone3d.pack_tone."""
        ds, st = self.dataset, self.dataset.store
        M = len(ds.contrast_list)
        classes = ds.FG_CLASSES.get(ds.dataset_name, ())
        col = ds.tone_col()
        tab, mask_host = self._table_head(metas, col + (tone3d.TONE_EXTRA(M) if ds.intensifies() else 0), (0, st.shape[2]), ds.aug)
        for r, (subj_id, _, _, _, tptr, _, _, _, (fg, u, flips, centre, *warp)) in enumerate(metas):
            if ds.intensifies():
                *warp, tone = warp
                tab[r, col:] = tone3d.pack_tone(*tone)
            flags = (patch3d.AUG if ds.aug else 0) | (patch3d.FG if fg else 0) | (patch3d.CENTRE if centre else 0)
            for axis, on in zip('hwd', flips):
                flags |= patch3d.FLIP_BITS[axis] if on else 0
            tab[r, 2 * M + 1] = flags
            if fg and tptr:
                tab[r, 2 * M + 3] = st.fg_prefix_ptr(subj_id + ds.TARGET_KEYS[ds.dataset_name], classes)
            w = np.asarray(u, dtype=np.uint32).astype(np.uint64)
            tab[r, 2 * M + 4] = (w[0] | (w[1] << np.uint64(32))).view(np.int64)
            tab[r, 2 * M + 5] = (w[2] | (w[3] << np.uint64(32))).view(np.int64)
            tab[r, 2 * M + 6] = w[4].view(np.int64)
            if warp and warp[0]:
                tab[r, 2 * M + 1] |= patch3d.WARP
                tab[r, 2 * M + 7:2 * M + 12] = patch3d.pack_warp(patch3d.warp_matrix(warp[1], warp[2]))
        return tab, mask_host

    def plain_plan(self, limit=None):
        """host half of the windowed reads: yields (batch index, dataset indices, item metas) of this rank's batches with every item as stored
        (VolumeDataset3D.meta(plain=True): nothing dropped, nothing augmented).  The batches follow the DATASET order whether or not the loader
        shuffles, and every subject is served (no equal_steps tail is dropped): the plan draws from no random stream, so every call gives the
        same batches -- all depth windows of a prediction see the same subjects in the same rows -- and a training loader's shuffle stream
        is left where it was.  For a loader that does not shuffle (the evaluation loaders) these are the batches of `batch_plan`."""
        n, bs = len(self.dataset), self.batch_size
        g = (n + bs - 1) // bs
        for k in range(g if limit is None else min(g, limit)):
            if k % self.world == self.rank:
                idxs = list(range(k * bs, min((k + 1) * bs, n)))
                yield k, idxs, [self.dataset.meta(i, plain=True) for i in idxs]

    @staticmethod
    def target_ptrs(batch):
        """(B,) int64 on the device: the addresses of a windowed batch's raw (H, W, D) label volumes, 0 = none -- word [2M] of its gather table
        (what hip.seg_label_volume scores a whole-volume prediction against).  Only the batches of `window` / `batches(z0=...)` carry the table."""
        table = batch['table']
        return table[:, (table.shape[1] - 3)].contiguous()

    def _upload(self, tab):
        dev = self.dataset.store.device
        host = torch.from_numpy(tab)
        if dev.type == 'cuda':
            host = host.pin_memory()
        return host.to(dev, non_blocking=True)                        # one small H2D copy per batch

    def _sample(self, k, metas, mask_host, gather):
        """the sample dict of a batch: `gather()` -> inputs and mask, `gather(targets=True, K=, relabel=)` -> targets; one launch each"""
        inputs, mask = gather()
        targets = gather(targets=True, K=self.region_channels, relabel=self.dataset.dataset_name == 'BraTS')
        return {'inputs': inputs, 'targets': targets, 'subj_id': [m[0] for m in metas],
                'slice_idx': torch.zeros(len(metas), dtype=torch.int64, device=self.dataset.store.device), 'mask': mask, 'mask_host': mask_host,
                'batch_index': k}

    def _gather(self, k, metas, z0, plain):
        ds, st = self.dataset, self.dataset.store
        H, W, D = st.shape
        M = len(ds.contrast_list)
        Dz = ds.crop()[1]
        tab, mask_host = self.table(metas, plain=plain)
        d = self._upload(tab)
        batch = self._sample(k, metas, mask_host, lambda **kw: hip.volume_gather(d, M, H, W, D, z0, Dz, **kw))
        if plain:
            batch['table'] = d                                        # windowed reads only: `target_ptrs` reads the label-volume addresses from it
        return batch

    def _gather_patch(self, k, metas):
        ds, st = self.dataset, self.dataset.store
        M = len(ds.contrast_list)
        tab, mask_host = self.patch_table(metas)
        d = self._upload(tab)
        classes = ds.FG_CLASSES.get(ds.dataset_name, ()) if ds.patch_fg > 0 else ()
        origins = patch3d.patch_origins(d, M, st.shape, ds.patch_size, classes)
        gather = patch3d.patch_warp if ds.warps() else patch3d.patch_gather
        batch = self._sample(k, metas, mask_host, lambda **kw: gather(d, origins, M, st.shape, ds.patch_size, **kw))
        batch['origins'] = origins
        if ds.intensifies():                                          # blur, statistics, tone: three more calls, on the inputs only
            batch['inputs'] = tone3d.patch_intensify(batch['inputs'], d, ds.tone_col(), M)
        return batch

    def window(self, k, metas, z0, flip=False):
        """one batch of `plain_plan` at depth offset z0 (same Dz as the crop), every item as stored, H-flipped by the gather itself if `flip`:
        the sample dict of `batches` plus 'table', the device gather table (`target_ptrs`)."""
        D = self.dataset.store.shape[2]
        Dz = self.dataset.crop()[1]
        if not 0 <= int(z0) <= D - Dz:
            raise ValueError(f'z0 {z0} outside [0, {D - Dz}] (D {D}, Dz {Dz})')
        if flip:
            metas = [m[:5] + (True,) + m[6:] for m in metas]
        return self._gather(k, metas, int(z0), plain=True)

    def tile(self, k, metas, origin, flips=0, tile=None):
        """one batch of `plain_plan` at tile origin (h0, w0, d0), every item as stored, mirrored by the gather itself along the axes of `flips`
        (patch3d.FLIP_H | FLIP_W | FLIP_D): the inputs and mask of `batches` (no targets: a prediction scores against the whole label volumes)
        plus 'table' (`target_ptrs`) and 'origins'.  `tile`: (TH, TW, TD), None: the dataset's patch_size.  The existing mrdis_patch_gather
        serves it: the augment bit is clear, the flip bits sit in the flag word, and the (B, 4) origins are written here, by the host
        (model3d.predict_tiles)."""
        ds, st = self.dataset, self.dataset.store
        M = len(ds.contrast_list)
        tile = ds.patch_size if tile is None else tile
        try:
            ok = len(tile) == 3 and len(origin) == 3 and all(int(v) == v for v in tuple(tile) + tuple(origin))
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError(f'tile {tile!r} at origin {origin!r}: two triples of integers (a loader without patch_size needs `tile`)')
        tile, origin = tuple(int(v) for v in tile), tuple(int(v) for v in origin)
        if any(not (1 <= t <= n and 0 <= o <= n - t) for t, o, n in zip(tile, origin, st.shape)):
            raise ValueError(f'tile {tile} at origin {origin} does not lie inside the stored volumes {tuple(st.shape)}')
        if isinstance(flips, bool) or not isinstance(flips, int) or flips & ~(patch3d.FLIP_H | patch3d.FLIP_W | patch3d.FLIP_D):
            raise ValueError(f'flips {flips!r}: bits of FLIP_H | FLIP_W | FLIP_D = {patch3d.FLIP_H | patch3d.FLIP_W | patch3d.FLIP_D}')
        tab, mask_host = self._table_head(metas, 2 * M + patch3d.TABLE_EXTRA, None, False)
        tab[:, 2 * M + 1] = flips
        d = self._upload(tab)
        origins = self._upload(np.array([origin + (-1,)] * len(metas), dtype=np.int32))
        inputs, mask = patch3d.patch_gather(d, origins, M, st.shape, tile)
        return {'inputs': inputs, 'subj_id': [m[0] for m in metas], 'slice_idx': torch.zeros(len(metas), dtype=torch.int64, device=st.device),
                'mask': mask, 'mask_host': mask_host, 'batch_index': k, 'origins': origins,
                'table': d[:, :2 * M + 3]}                            # the words every gather table starts with: `target_ptrs` reads [2M]

    def batches(self, limit=None, z0=None, flip=False):
        """`z0=None`: the reference's batches (crop [45:-46], drop-off, augmentation) -- in patch mode the patch batches.  An integer serves the batches of `plain_plan` with that
        depth offset and the same Dz, every item as stored (no drop-off redraws, no augmentation, no shuffle): the windowed reads for
        whole-volume prediction (model3d.predict_volumes).  `flip` (with z0 only): every item H-flipped by the gather itself."""
        if z0 is None:
            if flip:
                raise ValueError('flip belongs to the windowed reads: give z0')
            if self.dataset.patch_size is not None:
                for k, _, metas in self.batch_plan(limit):
                    yield self._gather_patch(k, metas)
                return
            crop_z0 = self.dataset.crop()[0]
            for k, _, metas in self.batch_plan(limit):
                yield self._gather(k, metas, crop_z0, plain=False)
        else:
            D = self.dataset.store.shape[2]
            Dz = self.dataset.crop()[1]
            if not 0 <= int(z0) <= D - Dz:
                raise ValueError(f'z0 {z0} outside [0, {D - Dz}] (D {D}, Dz {Dz})')
            for k, _, metas in self.plain_plan(limit):
                yield self.window(k, metas, z0, flip)


class VolumeData3D:
    """ZeroDoseDataAll3D (util.py:812-843): the three loaders of a fold.  `aug` reaches the train loader only and `dropoff` not the test loader
    (util.py:833-835).  The volumes come from `store` (a VolumeStore3D) or, without one, from the reference's h5 file under `data_path`."""

    @staticmethod
    def file_names(dataset_name, norm_type='mean', fold=0):
        """-> (h5 file, train list, val list, test list), util.py:814-829.  Any other dataset name raises (the reference leaves `data` unbound)."""
        if dataset_name == 'BraTS':
            h5 = 'BraTS_All.h5' if norm_type == 'mean' else 'BraTS_All_zscore_10.h5'
            return (h5,) + tuple(f'fold_BraTS_3d_{fold}_{s}_noval.txt' for s in ('train', 'val', 'test'))
        if dataset_name == 'ZeroDose':
            h5 = 'ZeroDose_FDG_All_1103_norm.h5' if norm_type == 'mean' else 'ZeroDose_FDG_All_1103_zscore_10.h5'
            return (h5,) + ('ZeroDose_3d_all.txt',) * 3
        raise ValueError(f'no 3-D dataset {dataset_name!r}: BraTS or ZeroDose')

    def __init__(self, dataset_name, data_path, norm_type='mean', batch_size=16, fold=0, shuffle=True, contrast_list=('T1',), aug=False,
                 dropoff=False, store=None, device='cuda:0', rank=0, world=1, generator=None, region_channels=0, patch_size=None, patch_fg=0.0,
                 patch_flips='h', patch_warp=0.0, patch_rot=(30, 30, 30), patch_zoom=(0.7, 1.4), **intensity):
        h5, *lists = self.file_names(dataset_name, norm_type, fold)
        if store is None:
            store = VolumeStore3D.from_h5(os.path.join(data_path, h5), device)
        self.store = store
        subj = [load_subj_list(os.path.join(data_path, f)) for f in lists]
        # patch mode: random patches for the train loader, the centre patch (no draw, no foreground share, no warp, no intensity change) for the
        # evaluation loaders
        intensity = patch_intensity_args(**intensity)
        mk = lambda s, a, d, centre: VolumeDataset3D(dataset_name, store, s, contrast_list=contrast_list, aug=a, dropoff=d, patch_size=patch_size,
                                                     patch_fg=0.0 if centre else patch_fg, patch_flips=patch_flips, patch_centre=centre,
                                                     patch_warp=0.0 if centre else patch_warp, patch_rot=patch_rot, patch_zoom=patch_zoom,
                                                     **({} if centre else intensity))
        kw = dict(rank=rank, world=world, generator=generator, region_channels=region_channels)
        self.trainLoader = VolumeLoader3D(mk(subj[0], aug, dropoff, False), batch_size, shuffle=shuffle, equal_steps=True, **kw)
        self.valLoader = VolumeLoader3D(mk(subj[1], False, dropoff, True), batch_size, shuffle=False, **kw)
        self.testLoader = VolumeLoader3D(mk(subj[2], False, False, True), batch_size, shuffle=False, **kw)
