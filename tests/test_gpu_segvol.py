"""Whole-volume sliding-window prediction on the GPU: the two kernels of csrc/mrdis_segvol.hip (hip.seg_accum, hip.seg_label_volume),
model3d.predict_volumes and `Run3D` with phase=predict.

Which shape takes which kernel path (see the header of mrdis_segvol.hip: a lane owns one ALIGNED group of four acc floats / four voxels; groups
cut by the start or end of a run / a sample go element by element):
  main      B 2, C 3, 5 x 6 x 37, Dz 16, offsets 0 8 16 21: a column is 111 floats, so the window of column k starts at phase (111 k + 3 z0) % 4
            -- every phase occurs in every launch: vector groups inside the runs, element groups at both ends.  H W D = 1110, % 4 = 2: the
            label kernel takes vector groups inside a sample and element groups where sample 0 ends and sample 1 starts.
  c1        B 3, C 1, same volume: column 37 floats, all phases again; samples start at voxel phases 0, 2, 0.
  elements  B 1, C 1, 3 x 5 x 7, Dz 3: a run of 3 floats never fills a group -- the accumulation's element path alone; H W D = 105: the
            label kernel's last group is partial.
  vectors   B 2, C 4, 4 x 6 x 16, Dz 8, offsets 0 8: every run starts and ends on a group boundary and H W D % 4 == 0 -- the vector paths alone.

Tolerances.  The accumulation has none fixed in advance: the fp32 torch composition (torch.sigmoid, += in the same order) is measured against
the float64 sum of float64 sigmoids in the same test, and the kernel may be at most twice as far off.  Labels and counts against the float64
oracle may disagree only at EXCUSED voxels -- some |pbar_c - 0.5| < 1e-6, or the two largest pbar within 1e-6 of each other -- and at most
1e-3 of the voxels may be excused (asserted on the CPU from the oracle alone, before the kernel's output is looked at).  With one window,
cover 1 and logits that are well separated, everything is exact."""
import os

import numpy as np
import pytest
import torch

from fixtures_data3d import data3d_volumes, data3d_subjects

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
EXCUSE = 1e-6
EXCUSED_SHARE = 1e-3

CASES = {
    'main': dict(B=2, C=3, H=5, W=6, D=37, Dz=16, offsets=[0, 8, 16, 21]),
    'c1': dict(B=3, C=1, H=5, W=6, D=37, Dz=16, offsets=[0, 8, 16, 21]),
    'elements': dict(B=1, C=1, H=3, W=5, D=7, Dz=3, offsets=[0, 2, 4]),
    'vectors': dict(B=2, C=4, H=4, W=6, D=16, Dz=8, offsets=[0, 8]),
}


# ----------------------------------------------------------------------------------------------- oracle (CPU, float64) and inputs
def make_case(name, seed=11, labels_max=3):
    """seeded CPU inputs of a case: one (B, H, W, Dz, C) logits tensor per (offset, flip), 3 * randn, and raw (B, H, W, D) label volumes"""
    c = dict(CASES[name])
    g = torch.Generator().manual_seed(seed)
    c['geom'] = [(z0, f) for z0 in c['offsets'] for f in (False, True)]
    c['logits'] = [3 * torch.randn(c['B'], c['H'], c['W'], c['Dz'], c['C'], generator=g) for _ in c['geom']]
    c['tvol'] = torch.randint(0, labels_max + 1, (c['B'], c['H'], c['W'], c['D']), generator=g).float()
    return c


def cover_of(c, geom):
    cover = torch.zeros(c['D'], dtype=torch.int32)
    for z0, _ in geom:
        cover[z0:z0 + c['Dz']] += 1
    return cover


def oracle_acc(c, geom, logits, dtype=torch.float64):
    """sum of sigmoids in `dtype`, in launch order, un-flipped, on the CPU: (B, H, W, D, C)"""
    acc = torch.zeros(c['B'], c['H'], c['W'], c['D'], c['C'], dtype=dtype)
    for (z0, f), l in zip(geom, logits):
        p = torch.sigmoid(l.to(dtype))
        acc[:, :, :, z0:z0 + c['Dz']] += p.flip(1) if f else p
    return acc


def oracle_labels_counts(acc64, cover, tvol, relabel):
    """float64 rule on the CPU -> labels (B, H, W, D) int64, per-voxel predicted / labelled masks (B, H, W, D, C), excused voxels (B, H, W, D)"""
    cov = cover.double().view(1, 1, 1, -1, 1)
    pbar = torch.where(cov > 0, acc64 / cov.clamp(min=1), torch.zeros_like(acc64))
    C = acc64.shape[-1]
    t = tvol.clone()
    if relabel:
        t[t == 4] = 3
    pred = pbar > 0.5
    lab = torch.stack([t == c + 1 for c in range(C)], dim=-1)
    arg = torch.from_numpy(np.argmax(pbar.numpy(), axis=-1))                       # numpy: the first maximum
    mx = pbar.max(dim=-1).values
    labels = torch.where(mx > 0.5, arg + 1, torch.zeros_like(arg))
    if relabel:
        labels[labels == 3] = 4
    excused = ((pbar - 0.5).abs() < EXCUSE).any(-1)
    if C > 1:
        top = pbar.topk(2, dim=-1).values
        excused |= (top[..., 0] - top[..., 1]) < EXCUSE
    excused &= (cover > 0).view(1, 1, 1, -1)                                       # nothing is decided where nothing was predicted
    return labels, pred, lab, excused


def counts_of(pred, lab, keep):
    """(B, C, 3) [I, P, T] over the voxels `keep` (B, H, W, D)"""
    k = keep.unsqueeze(-1)
    f = lambda m: (m & k).flatten(1, 3).sum(1)
    return torch.stack([f(pred & lab), f(pred), f(lab)], dim=-1)


def run_kernels(mrdis, c, geom, logits, relabel=False, tvol='own', cover=None):
    """the kernels on the device: acc, labels, counts (all back on the CPU) and the tensors that must stay alive"""
    hip = mrdis.hip
    acc = torch.zeros(c['B'], c['H'], c['W'], c['D'], c['C'], device=DEV)
    for (z0, f), l in zip(geom, logits):
        hip.seg_accum(l.to(DEV).permute(0, 4, 1, 2, 3), acc, z0, flip_h=f)
    vols = None
    ptrs = None
    if tvol is not None:
        vols = [v.contiguous().to(DEV) for v in (c['tvol'] if isinstance(tvol, str) else tvol)]
        ptrs = torch.tensor([v.data_ptr() for v in vols], dtype=torch.int64).to(DEV)
    cover = (cover_of(c, geom) if cover is None else cover).to(DEV)
    labels, counts = hip.seg_label_volume(acc, cover, ptrs, relabel=relabel)
    torch.cuda.synchronize()
    del vols
    return acc.cpu(), labels.cpu(), counts.cpu()


def assert_labels_counts(labels, counts, want_labels, pred, lab, excused, what):
    n_exc = int(excused.sum())
    assert n_exc <= EXCUSED_SHARE * excused.numel(), f'{what}: {n_exc} of {excused.numel()} voxels excused'
    bad = (labels.long() != want_labels) & ~excused
    assert int(bad.sum()) == 0, f'{what}: {int(bad.sum())} labels differ outside the excused voxels'
    lo = counts_of(pred, lab, ~excused)
    hi = lo + excused.flatten(1).sum(1).view(-1, 1, 1)
    assert bool(((counts >= lo) & (counts <= hi)).all()), f'{what}: counts {counts.tolist()} outside [{lo.tolist()}, {hi.tolist()}]'
    assert torch.equal(counts[..., 2].long(), counts_of(pred, lab, torch.ones_like(excused))[..., 2]), what      # T never depends on a probability


# ----------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize('name', list(CASES))
def test_accumulation_within_twice_the_torch_error_of_float64(mrdis, name):
    c = make_case(name)
    acc64 = oracle_acc(c, c['geom'], c['logits'])
    acc32 = torch.zeros(c['B'], c['H'], c['W'], c['D'], c['C'], device=DEV)        # the fp32 torch composition, same order, on the device
    for (z0, f), l in zip(c['geom'], c['logits']):
        p = torch.sigmoid(l.to(DEV))
        acc32[:, :, :, z0:z0 + c['Dz']] += p.flip(1) if f else p
    acc, _, _ = run_kernels(mrdis, c, c['geom'], c['logits'])
    e_torch = float((acc32.cpu().double() - acc64).abs().max())
    e_kernel = float((acc.double() - acc64).abs().max())
    print(f'\n[segvol accum {name}] max |acc - float64|: kernel {e_kernel:.3e}  torch fp32 composition {e_torch:.3e}  (max acc {float(acc64.max()):.2f})')
    assert e_torch > 0
    assert e_kernel <= 2 * e_torch
    outside = cover_of(c, c['geom']) == 0
    assert float(acc[:, :, :, outside].abs().max() if outside.any() else 0.0) == 0.0


@pytest.mark.parametrize('name', list(CASES))
def test_all_windows_and_flips_against_the_float64_oracle(mrdis, name):
    c = make_case(name)
    cover = cover_of(c, c['geom'])
    want, pred, lab, excused = oracle_labels_counts(oracle_acc(c, c['geom'], c['logits']), cover, c['tvol'], relabel=False)
    assert int(excused.sum()) <= EXCUSED_SHARE * excused.numel()                   # a condition on the inputs, from the oracle alone
    assert len(set(want.flatten().tolist())) == c['C'] + 1                         # every label occurs
    _, labels, counts = run_kernels(mrdis, c, c['geom'], c['logits'])
    assert labels.dtype == torch.uint8 and tuple(labels.shape) == (c['B'], c['H'], c['W'], c['D'])
    assert counts.dtype == torch.int32 and tuple(counts.shape) == (c['B'], c['C'], 3)
    assert_labels_counts(labels, counts, want, pred, lab, excused, name)


def separated_logits(c, g):
    """(B, H, W, Dz, C): |logit| <= 6, the channels of a voxel at least 0.02 apart, no logit within 1e-3 of 0: fp32 sigmoid keeps their order and side"""
    shape = (c['B'], c['H'], c['W'], c['Dz'])
    base = 9 * torch.rand(*shape, generator=g) - 4.5
    gaps = 0.02 + 0.4 * torch.rand(*shape, c['C'], generator=g)
    steps = gaps.cumsum(-1) - gaps[..., :1]                                        # 0, g1, g1 + g2, ...
    perm = torch.rand(*shape, c['C'], generator=g).argsort(-1)
    l = (base.unsqueeze(-1) + steps.gather(-1, perm)).float()
    l = torch.where(l.abs() < 1e-3, torch.full_like(l, 1e-3), l)
    s = l.sort(-1).values
    assert float(l.abs().max()) <= 6 and float(l.abs().min()) >= 1e-3
    assert c['C'] == 1 or float((s[..., 1:] - s[..., :-1]).min()) >= 0.01
    return l


def test_one_window_is_exact(mrdis):
    c = make_case('main')
    g = torch.Generator().manual_seed(5)
    z0 = 21                                                                        # odd: the runs start at every phase
    l = separated_logits(c, g)
    # planted: exact ties (the lowest channel wins) and exact zeros (sigmoid(0) == 0.5 is NOT above 0.5)
    l[0, 0, 0, 0] = torch.tensor([2.0, 2.0, 1.0]); l[0, 0, 1, 1] = torch.tensor([-1.0, 1.5, 1.5]); l[1, 4, 5, 15] = torch.tensor([0.75, 0.75, 0.75])
    l[0, 2, 3, 4] = torch.tensor([0.0, 0.0, 0.0]); l[1, 1, 1, 7] = torch.tensor([-2.0, 0.0, -1.0]); l[1, 3, 2, 9] = torch.tensor([0.0, 3.0, 0.0])
    geom, logits = [(z0, False)], [l]
    acc, labels, counts = run_kernels(mrdis, c, geom, logits)
    # labels: the rule evaluated on the logits
    mx = l.max(-1).values
    arg = torch.from_numpy(np.argmax(l.numpy(), axis=-1))
    want = torch.zeros(c['B'], c['H'], c['W'], c['D'], dtype=torch.int64)
    want[:, :, :, z0:z0 + c['Dz']] = torch.where(mx > 0, arg + 1, torch.zeros_like(arg))
    assert torch.equal(labels.long(), want)
    assert labels[0, 0, 0, z0] == 1 and labels[0, 0, 1, z0 + 1] == 2 and labels[1, 4, 5, z0 + 15] == 1
    assert labels[0, 2, 3, z0 + 4] == 0 and labels[1, 1, 1, z0 + 7] == 0 and labels[1, 3, 2, z0 + 9] == 2
    # counts: mrdis_seg_counts of the window + the labelled voxels of the uncovered depths
    tw = c['tvol'][:, :, :, z0:z0 + c['Dz']]
    region = torch.stack([(tw == k + 1).float() for k in range(c['C'])], dim=-1)  # (B, H, W, Dz, C)
    ref = mrdis.hip.seg_counts(l.to(DEV).permute(0, 4, 1, 2, 3), region.to(DEV).permute(0, 4, 1, 2, 3), logits=True).cpu()
    outside = torch.ones(c['D'], dtype=torch.bool); outside[z0:z0 + c['Dz']] = False
    for k in range(c['C']):
        ref[:, k, 2] += (c['tvol'][:, :, :, outside] == k + 1).flatten(1).sum(1).int()
    assert torch.equal(counts, ref)


def test_relabel_zero_pointer_and_uncovered_depths(mrdis):
    c = make_case('main', labels_max=4)
    c['tvol'][c['tvol'] == 3] = 4                                                  # BraTS raw labels: 0 / 1 / 2 / 4
    geom, logits = c['geom'][:4], c['logits'][:4]                                  # offsets 0 and 8, both flips: depths 24 .. 36 stay uncovered
    cover = cover_of(c, geom)
    assert int((cover == 0).sum()) == 13
    want, pred, lab, excused = oracle_labels_counts(oracle_acc(c, geom, logits), cover, c['tvol'], relabel=True)
    assert int(excused.sum()) <= EXCUSED_SHARE * excused.numel()
    _, labels, counts = run_kernels(mrdis, c, geom, logits, relabel=True)
    assert_labels_counts(labels, counts, want, pred, lab, excused, 'relabel')
    assert set(labels.flatten().tolist()) == {0, 1, 2, 4}                          # a predicted channel 2 is written as 4
    assert int((labels[:, :, :, cover == 0] != 0).sum()) == 0                      # uncovered depths: label 0
    assert int(counts[:, 2, 2].sum()) == int((c['tvol'] == 4).sum()) > 0           # a 4 in the target counts under channel 2
    # without relabel the raw 4 matches no channel
    _, labels_raw, counts_raw = run_kernels(mrdis, c, geom, logits, relabel=False)
    assert int(counts_raw[:, 2, 2].sum()) == 0 and set(labels_raw.flatten().tolist()) == {0, 1, 2, 3}
    assert torch.equal(counts_raw[:, :, 1], counts[:, :, 1])
    # a zero target pointer: T = I = 0 for that sample, P and the labels unaffected
    hip = mrdis.hip
    acc = torch.zeros(c['B'], c['H'], c['W'], c['D'], c['C'], device=DEV)
    for (z0, f), l in zip(geom, logits):
        hip.seg_accum(l.to(DEV).permute(0, 4, 1, 2, 3), acc, z0, flip_h=f)
    v1 = c['tvol'][1].contiguous().to(DEV)
    ptrs = torch.tensor([0, v1.data_ptr()], dtype=torch.int64).to(DEV)
    labels0, counts0 = hip.seg_label_volume(acc, cover.to(DEV), ptrs, relabel=True)
    assert torch.equal(labels0.cpu(), labels)
    assert counts0[0, :, 0].tolist() == [0, 0, 0] and counts0[0, :, 2].tolist() == [0, 0, 0]
    assert torch.equal(counts0[:, :, 1].cpu(), counts[:, :, 1]) and torch.equal(counts0[1].cpu(), counts[1])
    labels_n, counts_n = hip.seg_label_volume(acc, cover.to(DEV), None, relabel=True)     # no targets at all
    assert torch.equal(labels_n.cpu(), labels) and int(counts_n[:, :, [0, 2]].abs().sum()) == 0


def test_launch_counters_and_bit_identical_runs(mrdis):
    c = make_case('main')
    before = mrdis.hip.launch_counts()
    a1 = run_kernels(mrdis, c, c['geom'], c['logits'])
    mid = mrdis.hip.launch_counts()
    assert mid['segaccum'] - before['segaccum'] == len(c['offsets']) * 2           # windows x flips
    assert mid['seglabels'] - before['seglabels'] == 1                             # one per batch
    a2 = run_kernels(mrdis, c, c['geom'], c['logits'])
    for x, y in zip(a1, a2):
        assert torch.equal(x, y)


def test_layouts_and_offsets_are_refused(mrdis):
    hip = mrdis.hip
    B, C, H, W, D, Dz = 2, 3, 5, 6, 37, 16
    acc = torch.zeros(B, H, W, D, C, device=DEV)
    good = torch.zeros(B, H, W, Dz, C, device=DEV).permute(0, 4, 1, 2, 3)
    hip.seg_accum(good, acc, D - Dz)
    with pytest.raises(hip.MrdisError):
        hip.seg_accum(good, acc, D - Dz + 1)                                       # z0 > D - Dz
    with pytest.raises(hip.MrdisError):
        hip.seg_accum(good, acc, -1)
    with pytest.raises(hip.MrdisError):
        hip.seg_accum(torch.zeros(B, C, H, W, Dz, device=DEV), acc, 0)             # contiguous NCDHW: not channels-last-3d
    with pytest.raises(hip.MrdisError):
        hip.seg_accum(torch.zeros(B, H, W, 2 * Dz, C, device=DEV)[:, :, :, ::2].permute(0, 4, 1, 2, 3), acc, 0)      # holes
    with pytest.raises(hip.MrdisError):
        hip.seg_accum(good, torch.zeros(B, H, W, D, 2 * C, device=DEV)[..., :C], 0)          # acc not dense
    with pytest.raises(hip.MrdisError):
        hip.seg_accum(good, torch.zeros(B, H, W, D, C + 1, device=DEV), 0)         # channel counts differ
    cover = torch.ones(D, dtype=torch.int32, device=DEV)
    with pytest.raises(hip.MrdisError):
        hip.seg_label_volume(acc.permute(0, 2, 1, 3, 4), cover)
    with pytest.raises(hip.MrdisError):
        hip.seg_label_volume(acc, cover.long())
    with pytest.raises(hip.MrdisError):
        hip.seg_label_volume(acc, torch.ones(2 * D, dtype=torch.int32, device=DEV)[::2])
    with pytest.raises(hip.MrdisError):
        hip.seg_label_volume(acc, cover, torch.zeros(B + 1, dtype=torch.int64, device=DEV))
    assert float(acc.sum()) == B * H * W * Dz * C * 0.5                            # only the one good call added (sigmoid(0) = 0.5)


# ----------------------------------------------------------------------------------------------- predict_volumes and Run3D
CONTRASTS = ['T1', 'T1c', 'T2', 'T2_FLAIR']


@pytest.fixture(scope='module')
def world(tmp_path_factory):
    """(store arrays, data_path with the three list files): 32 x 32 x 123 volumes (a contrast missing now and then reads as zeros); the reader serves all but the first
    line of a list (data3d.load_subj_list), so the test list's four subjects give three served ones: a batch of two and a batch of one"""
    data = data3d_volumes(n_subj=11, H=32, W=32, D=123, contrasts=CONTRASTS, seed=9)
    subj = data3d_subjects(data)
    root = tmp_path_factory.mktemp('segvol')
    for name, part in (('train', subj[:4]), ('val', subj[4:7]), ('test', subj[7:11])):
        (root / f'fold_BraTS_3d_0_{name}_noval.txt').write_text('\n'.join(part) + '\n')
    return data, str(root), subj[8:11]


def _data(mrdis, world):
    store = mrdis.VolumeStore3D.from_arrays(world[0], DEV)
    return mrdis.VolumeData3D('BraTS', world[1], norm_type='z-score', batch_size=2, fold=0, shuffle=True, contrast_list=CONTRASTS, aug=True,
                              dropoff=True, store=store, device=DEV, region_channels=3)


def _model(mrdis, seed=3, symmetric=False):
    torch.manual_seed(seed)
    model = mrdis.NVNet3D((32, 32, 32), 4, 3, 8, p=0.2).to(DEV)
    if symmetric:                                                                  # H is the first kernel axis of every Conv3d here
        with torch.no_grad():
            for m in model.unet.modules():
                if isinstance(m, mrdis.HipConv3d) and m.kernel_size == (3, 3, 3):
                    w = m.weight
                    if m.stride == (2, 2, 2):                                      # out[o] = f(in[2o], in[2o + 1]): the pair a flip maps onto itself
                        mean = (w[:, :, 1] + w[:, :, 2]) / 2
                        w[:, :, 0] = 0; w[:, :, 1] = mean; w[:, :, 2] = mean
                    else:
                        w.copy_((w + w.flip(2)) / 2)
    return model


def _oracle_prediction(mrdis, model, loader, offsets, flips=(False,)):
    """plain torch float64 composition of the same windows: {subj_id: (acc64 (H, W, D, C) on the CPU)}"""
    H, W, D = loader.dataset.store.shape
    out = {}
    model.unet.eval()
    with torch.no_grad():
        for z0 in offsets:
            for batch in loader.batches(z0=z0):
                for f in flips:
                    x = batch['inputs'].flip(2).contiguous(memory_format=torch.channels_last_3d) if f else batch['inputs']
                    u = model.unet(x)[0]
                    p = torch.sigmoid(u.double())
                    if f:
                        p = p.flip(2)
                    p = p.permute(0, 2, 3, 4, 1).cpu()                             # (B, H, W, Dz, C)
                    for i, sid in enumerate(batch['subj_id']):
                        a = out.setdefault(sid, torch.zeros(H, W, D, p.shape[-1], dtype=torch.float64))
                        a[:, :, z0:z0 + p.shape[3]] += p[i]
    return out


def _collect(gen):
    res = {'subj_id': [], 'labels': [], 'counts': [], 'acc': []}
    for r in gen:
        res['subj_id'] += r['subj_id']
        for k in ('labels', 'counts', 'acc'):
            res[k].append(r[k].cpu())
    return {k: (v if k == 'subj_id' else torch.cat(v)) for k, v in res.items()}


@pytest.fixture(scope='module')
def predicted(mrdis, world):
    data = _data(mrdis, world)
    model = _model(mrdis)
    before = mrdis.hip.launch_counts()
    res = _collect(mrdis.predict_volumes(model, data.testLoader, stride=16))
    after = mrdis.hip.launch_counts()
    return data, model, res, {k: after[k] - before[k] for k in ('segaccum', 'seglabels')}


def test_predict_volumes_equals_the_float64_composition(mrdis, world, predicted):
    data, model, res, launches = predicted
    offsets = mrdis.window_offsets(123, 32, 16)
    assert offsets[-1] == 91 and len(offsets) == 7
    assert res['subj_id'] == world[2] and launches == {'segaccum': 7 * 2, 'seglabels': 2}            # two batches (2 + 1 subjects) x 7 windows
    assert res['labels'].dtype == torch.uint8 and tuple(res['labels'].shape) == (3, 32, 32, 123)
    assert tuple(res['counts'].shape) == (3, 3, 3)
    assert model.training                                                          # the mode the caller had is put back
    acc64 = _oracle_prediction(mrdis, model, data.testLoader, offsets)
    acc64 = torch.stack([acc64[s] for s in res['subj_id']])
    tvol = torch.stack([torch.from_numpy(np.asarray(world[0][s + '/seg'], dtype=np.float32)) for s in res['subj_id']])
    cover = torch.from_numpy(mrdis.model3d.window_cover(123, 32, offsets))
    want, pred, lab, excused = oracle_labels_counts(acc64, cover, tvol, relabel=True)
    print(f'\n[segvol predict_volumes] excused voxels {int(excused.sum())} of {excused.numel()}, predicted share {float(pred.double().mean()):.3f}, '
          f'max |acc - float64| {float((res["acc"].double() - acc64).abs().max()):.3e}')
    assert_labels_counts(res['labels'], res['counts'], want, pred, lab, excused, 'predict_volumes')
    assert set(res['labels'].flatten().tolist()) <= {0, 1, 2, 4}


def test_nvnet_and_its_unet_predict_the_same_bits(mrdis, predicted):
    data, model, res, _ = predicted
    alone = _collect(mrdis.predict_volumes(model.unet, data.testLoader, stride=16))
    assert torch.equal(alone['labels'], res['labels']) and torch.equal(alone['counts'], res['counts']) and torch.equal(alone['acc'], res['acc'])


def test_flip_changes_the_accumulator_but_not_a_symmetric_net(mrdis, world, predicted):
    data, model, res, _ = predicted
    flipped = _collect(mrdis.predict_volumes(model, data.testLoader, stride=16, flip=True))
    assert not torch.equal(flipped['acc'] / 2, res['acc'])                         # a generic net is not H-symmetric
    sym = _model(mrdis, symmetric=True)
    offsets = mrdis.window_offsets(123, 32, 16)
    a = _collect(mrdis.predict_volumes(sym, data.testLoader, stride=16))
    b = _collect(mrdis.predict_volumes(sym, data.testLoader, stride=16, flip=True))
    acc64 = _oracle_prediction(mrdis, sym, data.testLoader, offsets)
    acc64 = torch.stack([acc64[s] for s in a['subj_id']])
    tvol = torch.stack([torch.from_numpy(np.asarray(world[0][s + '/seg'], dtype=np.float32)) for s in a['subj_id']])
    _, _, _, excused = oracle_labels_counts(acc64, torch.from_numpy(mrdis.model3d.window_cover(123, 32, offsets)), tvol, relabel=True)
    assert int(excused.sum()) <= EXCUSED_SHARE * excused.numel()
    differ = (a['labels'] != b['labels']) & ~excused
    print(f'\n[segvol flip, H-symmetric net] excused {int(excused.sum())}, labels that differ outside them {int(differ.sum())}, '
          f'max |acc_flip / 2 - acc| {float((b["acc"] / 2 - a["acc"]).abs().max()):.3e}')
    assert int(differ.sum()) == 0


def test_loader_refusals_and_windowed_batches(mrdis, world):
    data = _data(mrdis, world)
    model = _model(mrdis)
    with pytest.raises(ValueError):
        next(mrdis.predict_volumes(model, data.trainLoader))                       # aug
    with pytest.raises(ValueError):
        next(mrdis.predict_volumes(model, data.valLoader))                         # drop-off
    with pytest.raises(ValueError):
        next(data.testLoader.batches(z0=92))
    a, b = list(data.testLoader.batches()), list(data.testLoader.batches(z0=None))
    assert len(a) == len(b) == 2
    assert 'table' not in a[0] and 'table' not in b[0]                             # the ordinary batches are what they were, key for key
    for x, y in zip(a, b):
        assert x['subj_id'] == y['subj_id']
        for k in ('inputs', 'targets', 'mask'):
            assert torch.equal(x[k], y[k]) and x[k].stride() == y[k].stride()
    w = list(data.testLoader.batches(z0=45))                                       # the crop's own offset, read as stored: the same tensors again
    for x, y in zip(a, w):
        assert torch.equal(x['inputs'], y['inputs']) and torch.equal(x['targets'], y['targets'])
    f = list(data.testLoader.batches(z0=91, flip=True))
    p = list(data.testLoader.batches(z0=91))
    assert torch.equal(f[0]['inputs'], p[0]['inputs'].flip(2))
    sid = w[0]['subj_id'][0]
    assert set(w[0]) == set(a[0]) | {'table'}                                      # the windowed batches add the gather table
    assert int(data.testLoader.target_ptrs(w[0])[0]) == data.store.ptr(sid + '/seg')


RUN_CFG = dict(dataset_name='BraTS', contrast_list=CONTRASTS, batch_size=2, model_name='NVNet3D', init_channels=8, epochs=1, lr=1e-4,
               device='cuda:0', seed=10)


@pytest.fixture(scope='module')
def trained(mrdis, world, tmp_path_factory):
    """(config, store) of a one-epoch run that left model_best.pth.tar under its ckpt_path"""
    cfg = dict(RUN_CFG, data_path=world[1], ckpt_path=str(tmp_path_factory.mktemp('ckpt')))
    store = mrdis.VolumeStore3D.from_arrays(world[0], DEV)
    mrdis.Run3D(cfg, store=store, log=lambda *a: None).train()
    return cfg, store


def test_run3d_phase_predict_writes_label_volumes_and_csv(mrdis, world, trained):
    cfg, store = trained
    run = mrdis.Run3D(dict(cfg, phase='predict', predict_stride=16), store=store, log=lambda *a: None)
    assert run.start_epoch == 0
    stat = run.predict()
    out = os.path.join(cfg['ckpt_path'], 'result_test')
    assert sorted(os.listdir(out)) == sorted([f'{s}_seg.npy' for s in world[2]] + ['predict.csv'])
    for s in world[2]:
        v = np.load(os.path.join(out, f'{s}_seg.npy'))
        assert v.dtype == np.uint8 and v.shape == (32, 32, 123) and set(np.unique(v).tolist()) <= {0, 1, 2, 4}
    res = _collect(mrdis.predict_volumes(run.model, run.loaders['test'], stride=16))
    met = mrdis.seg_metrics_from_counts(res['counts'].numpy())
    rows = open(os.path.join(out, 'predict.csv')).read().splitlines()
    assert rows[0] == 'subj_id,dice,iou' and len(rows) == 4
    for row, s, d, i in zip(rows[1:], res['subj_id'], met['dice'].tolist(), met['iou'].tolist()):
        sid, dice, iou = row.split(',')
        assert sid == s and float(dice) == d and float(iou) == i
    for s, lab in zip(res['subj_id'], res['labels']):
        assert np.array_equal(np.load(os.path.join(out, f'{s}_seg.npy')), lab.numpy())
    assert stat['n'] == 3 and np.isfinite(stat['dice']) and np.isfinite(stat['iou'])
    assert stat['dice'] == pytest.approx(float(met['dice'].mean()), abs=1e-12) and stat['iou'] == pytest.approx(float(met['iou'].mean()), abs=1e-12)


def test_predicting_a_shuffling_train_loader_keeps_every_subject_in_its_own_volume(mrdis, world, trained):
    """`predict_set: train` goes through Run3D's train loader, which shuffles: every window of a batch must still gather the same subjects (one
    plan, drawn once, in dataset order), so each <subj>_seg.npy and predict.csv row equals what an unshuffled loader over the same list gives
    for that subject, bit for bit; and predicting leaves the shuffle stream where it was"""
    cfg, store = trained
    run = mrdis.Run3D(dict(cfg, phase='predict', predict_set='train', predict_stride=16, aug=False, dropoff=False), store=store,
                      log=lambda *a: None)
    loader = run.loaders['train']
    assert loader.shuffle and not loader.dataset.aug and not loader.dataset.dropoff
    served = [str(s) for s in loader.dataset.subj_list]
    assert len(served) == 3                                                        # the list's four lines minus the one read as a header
    rng_before = torch.get_rng_state()
    stat = run.predict()
    assert torch.equal(torch.get_rng_state(), rng_before)                          # no draw from the stream the training shuffles come from
    plain = mrdis.VolumeLoader3D(loader.dataset, 2, shuffle=False, region_channels=3)
    want = _collect(mrdis.predict_volumes(run.model, plain, stride=16))
    assert want['subj_id'] == served
    assert len({want['labels'][i].numpy().tobytes() for i in range(3)}) == 3       # the subjects' volumes differ: a mix-up would show
    out = os.path.join(cfg['ckpt_path'], 'result_train')
    met = mrdis.seg_metrics_from_counts(want['counts'].numpy())
    rows = dict((r.split(',')[0], r.split(',')[1:]) for r in open(os.path.join(out, 'predict.csv')).read().splitlines()[1:])
    assert sorted(rows) == sorted(served) and stat['n'] == 3
    for i, s in enumerate(served):
        assert np.array_equal(np.load(os.path.join(out, f'{s}_seg.npy')), want['labels'][i].numpy()), s
        assert float(rows[s][0]) == float(met['dice'][i]) and float(rows[s][1]) == float(met['iou'][i]), s
    # the generator itself, twice over the shuffling loader: the same subjects, the same bits
    a = _collect(mrdis.predict_volumes(run.model, loader, stride=16, flip=True))
    b = _collect(mrdis.predict_volumes(run.model, loader, stride=16, flip=True))
    assert a['subj_id'] == b['subj_id'] == served and torch.equal(a['labels'], b['labels']) and torch.equal(a['acc'], b['acc'])
    # every window of a shuffling loader serves the same subjects
    ids = [[x['subj_id'] for x in loader.batches(z0=z0)] for z0 in (0, 16, 91)]
    assert ids[0] == ids[1] == ids[2] == [served[:2], served[2:]]
