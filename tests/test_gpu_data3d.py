"""The HBM-resident 3-D loader (data3d.py, csrc/mrdis_volgather.hip) on the GPU: every batch recorded from the reference's own
ZeroDoseDataset3D + DataLoader (tests/golden/data3d_b2.npz), both kernels of the gather on the same batches, odd geometries against a plain
torch composition, launch counts, region-channel targets, two NVNet3D optimizer steps fed by the loader, and replay through a HIP graph."""
import os

import numpy as np
import pytest
import torch

from fixtures_data3d import DATA3D_CFG, data3d_volumes, data3d_subjects, compose_item, aug_bound

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
C = DATA3D_CFG


def _loader(mrdis, data, aug, subj=None, contrasts=None, batch_size=None, dropoff=True, shuffle=True, K=0, name='BraTS'):
    store = mrdis.VolumeStore3D.from_arrays(data, DEV)
    ds = mrdis.VolumeDataset3D(name, store, subj or data3d_subjects(data), contrasts or C['contrasts'], aug=aug, dropoff=dropoff)
    return mrdis.VolumeLoader3D(ds, batch_size or C['batch_size'], shuffle=shuffle, region_channels=K)


def _torch_batch(store, ds, metas, K=0):
    """the batch as a plain torch composition over the same store and the same draws (stack, slice, flip, mul / add, where, permute)"""
    H, W, D = store.shape
    z0, Dz = ds.crop()
    xs, ts = [], []
    for sid, _, ptrs, drop, tptr, flip, scale, shift in metas:
        vols = [store.vols.get(sid + '/' + c) if m != drop else None for m, c in enumerate(ds.contrast_list)]
        raw = torch.stack([v[:, :, z0:z0 + Dz] if v is not None else torch.zeros(H, W, Dz, device=DEV) for v in vols])
        tkey = ds.TARGET_KEYS.get(ds.dataset_name)
        seg = store.vols.get(sid + tkey) if tkey else None
        t = seg[:, :, z0:z0 + Dz] if seg is not None else torch.zeros(H, W, Dz, device=DEV)
        if ds.dataset_name == 'BraTS':
            t = torch.where(t == 4, torch.full_like(t, 3.0), t)
        if flip:
            raw, t = raw.flip(1), t.flip(0)
        x = raw
        if ds.aug:
            x = raw * float(np.float32(scale)) + float(np.float32(shift))
            x = torch.where(raw == raw.min(), torch.full_like(x, -10.0), x)
        xs.append(x); ts.append(t)
    x, t = torch.stack(xs), torch.stack(ts)
    if K:
        t = torch.stack([(t == c + 1).float() for c in range(K)], 1).contiguous(memory_format=torch.channels_last_3d)
    return x.contiguous(memory_format=torch.channels_last_3d), t.contiguous()


def _epochs(mrdis, gold, data, check):
    """walk the fixture's epochs with its seeds; check(kind, tag, loader, batch, metas) per batch"""
    la, ln = _loader(mrdis, data, True), _loader(mrdis, data, False)
    np.random.seed(C['np_seed']); torch.manual_seed(C['torch_seed'])
    n = 0
    for kind, loader, epochs in (('a', la, C['aug_epochs']), ('n', ln, C['plain_epochs'])):
        for ep in range(epochs):
            # batch_plan and batches draw alike: plan the epoch on a saved stream, then serve it
            st_np, st_t = np.random.get_state(), torch.get_rng_state()
            saved = loader._drop_rng
            plans = list(loader.batch_plan())
            np.random.set_state(st_np); torch.set_rng_state(st_t); loader._drop_rng = saved
            for bi, b in enumerate(loader):
                check(kind, f'{kind}{ep}_{bi}', loader, b, plans[bi][2])
                n += 1
            assert bi + 1 == int(gold[f'nbatch_{kind}{ep}'])
            assert np.random.rand() == float(gold[f'next_rand_{kind}{ep}'])
    assert n == 12
    return n


def test_every_recorded_batch_matches_the_reference(mrdis, golden_dir):
    """aug off: inputs and targets bit for bit.  aug on: |got - ref| <= 4 * 2^-24 * (|x| scale + |shift|) elementwise (fp32 x * scale + shift with
    fp32-rounded parameters against the reference's float64: two roundings plus the two parameter roundings; derived, not measured), the set
    of -10 identical, targets bit-equal.  Every element of every batch."""
    gold = np.load(os.path.join(golden_dir, 'data3d_b2.npz'))
    data = data3d_volumes()
    worst = [0.0]

    def check(kind, tag, loader, b, metas):
        x, t = b['inputs'], b['targets']
        assert x.is_contiguous(memory_format=torch.channels_last_3d) or x.shape[0] == 1
        assert x.permute(0, 2, 3, 4, 1).is_contiguous()
        x, t = x.cpu().numpy(), t.cpu().numpy()
        ref = gold[f'inputs_{tag}']
        assert x.shape == ref.shape and x.dtype == np.float32
        assert b['subj_id'] == list(gold[f'subj_{tag}'])
        np.testing.assert_array_equal(b['mask'].cpu().numpy(), gold[f'mask_{tag}'])
        np.testing.assert_array_equal(b['mask_host'], gold[f'mask_{tag}'])
        np.testing.assert_array_equal(b['slice_idx'].cpu().numpy(), gold[f'slice_{tag}'])
        np.testing.assert_array_equal(t, gold[f'targets_{tag}'])
        np.testing.assert_array_equal(x == -10, ref == -10)
        assert int((x == -10).sum()) == int(gold[f'insum_{tag}'][2])
        if kind == 'n':
            np.testing.assert_array_equal(x, ref)
            return
        z0, Dz = loader.dataset.crop()
        for r, (sid, _, ptrs, drop, tptr, flip, scale, shift) in enumerate(metas):
            _, raw, _ = compose_item(data, sid, C['contrasts'], drop, flip, scale, shift, True, z0, Dz)
            err, bound = np.abs(x[r].astype(np.float64) - ref[r]), aug_bound(raw, scale, shift)
            live = ref[r] != -10
            worst[0] = max(worst[0], float((err[live] / bound[live]).max()))
            assert (err[live] <= bound[live]).all(), (tag, r, float((err[live] / bound[live]).max()))

    _epochs(mrdis, gold, data, check)
    print(f'worst error / bound {worst[0]:.3f}')


def test_tile_and_element_kernels_agree_and_launch_once(mrdis, golden_dir):
    """the LDS-tile form and the element kernel, each forced on the fixture's batches, agree bit for bit (inputs, targets, region channels, masks);
    per batch the library launches exactly one gather for the inputs and one for the targets, and nothing else"""
    gold = np.load(os.path.join(golden_dir, 'data3d_b2.npz'))
    data = data3d_volumes()
    hip = mrdis.hip
    got = {}
    for gen in (0, 1):
        hip.set_option('debug_volgen', gen)
        out = got[gen] = []
        la = _loader(mrdis, data, True, K=3)
        np.random.seed(C['np_seed']); torch.manual_seed(C['torch_seed'])
        la.dataset.store.crop_min_ptr('none', *la.dataset.crop())            # the per-volume minima are made once, before the counted region
        for ep in range(2):
            it = iter(la)
            while True:
                hip.launch_counts(reset=True)
                b = next(it, None)
                if b is None:
                    break
                c = hip.launch_counts()
                assert c['volgather'] == 2 and c['all'] == 2, c
                out.append((b['inputs'].clone(), b['targets'].clone(), b['mask'].clone()))
    hip.set_option('debug_volgen', 0)
    assert len(got[0]) == len(got[1]) == 6
    for (x0, t0, m0), (x1, t1, m1) in zip(got[0], got[1]):
        assert torch.equal(x0, x1) and torch.equal(t0, t1) and torch.equal(m0, m1)
        assert t0.shape[1] == 3 and t0.permute(0, 2, 3, 4, 1).is_contiguous()
    x0 = got[0][0][0].cpu().numpy()
    np.testing.assert_array_equal(x0 == -10, gold['inputs_a0_0'] == -10)


@pytest.mark.parametrize('geom', [dict(M=3, H=17, W=23, D=96, B=1, K=0), dict(M=3, H=17, W=23, D=96, B=1, K=3), dict(M=1, H=5, W=3, D=92, B=2, K=2),
                                  dict(M=8, H=6, W=10, D=95, B=3, K=0), dict(M=16, H=4, W=6, D=103, B=2, K=4), dict(M=33, H=3, W=4, D=95, B=2, K=0),
                                  dict(M=5, H=9, W=8, D=99, B=2, K=1), dict(M=64, H=2, W=3, D=93, B=1, K=64)], ids=lambda g: '-'.join(f'{k}{v}' for k, v in g.items()))
def test_odd_geometries_against_torch(mrdis, geom):
    """odd sizes, M from 1 to 64, partial batches: inputs, targets and region channels equal the plain torch composition bit for bit, under the default
    policy and with the element kernel forced"""
    M, H, W, D, B, K = (geom[k] for k in 'MHWDBK')
    contrasts = [f'c{m}' for m in range(M)]
    data = data3d_volumes(n_subj=5, H=H, W=W, D=D, contrasts=contrasts, seed=11 + M)
    for gen in (0, 1):
        mrdis.hip.set_option('debug_volgen', gen)
        la = _loader(mrdis, data, True, contrasts=contrasts, batch_size=B, K=K)
        np.random.seed(3); torch.manual_seed(4)
        st_np, st_t = np.random.get_state(), torch.get_rng_state()
        plans = list(la.batch_plan())
        np.random.set_state(st_np); torch.set_rng_state(st_t)
        n = 0
        for b, (_, _, metas) in zip(la, plans):
            x, t = _torch_batch(la.dataset.store, la.dataset, metas, K)
            assert b['inputs'].shape == (len(metas), M, H, W, D - 91) and torch.equal(b['inputs'], x)
            assert b['targets'].shape == t.shape and torch.equal(b['targets'], t)
            n += 1
        assert n == (5 + B - 1) // B
    mrdis.hip.set_option('debug_volgen', 0)


def test_zerodose_crop_and_absent_targets(mrdis):
    """'ZeroDose' crops [45:-47] and takes '/PET' targets without relabelling; a dataset without a target key gets zeros"""
    data = data3d_volumes(n_subj=3, H=8, W=12, D=100)
    for sid in data3d_subjects(data):
        data[sid + '/PET'] = data.pop(sid + '/seg') + 0.5
    for name in ('ZeroDose', 'Tau'):
        la = _loader(mrdis, data, False, batch_size=3, shuffle=False, dropoff=False, name=name)
        (_, _, metas), = list(la.batch_plan())
        b, = list(la)
        x, t = _torch_batch(la.dataset.store, la.dataset, metas)
        assert b['inputs'].shape[-1] == (8 if name == 'ZeroDose' else 9)
        assert torch.equal(b['inputs'], x) and torch.equal(b['targets'], t)
        assert (float(b['targets'].max()) == 4.5) == (name == 'ZeroDose') and (name == 'ZeroDose' or float(b['targets'].abs().max()) == 0.0)


def test_two_optimizer_steps_fed_by_the_loader(mrdis):
    """two NVNet3D steps (forward, nvnet_loss on region channels, backward, ArenaAdam) fed by the loader equal the same steps fed by tensors built with
    plain torch ops from the same store and the same draws: bit-identical losses"""
    H, W, D = 16, 32, 107                          # Dz = 16: VAEBranch wants every dimension a multiple of 16
    data = data3d_volumes(n_subj=4, H=H, W=W, D=D, seed=9)
    losses = {}
    for fed in ('loader', 'torch'):
        la = _loader(mrdis, data, True, batch_size=2, K=3)
        torch.manual_seed(10); np.random.seed(10)
        model = mrdis.NVNet3D((H, W, D - 91), 4, 3, 8, p=0.0).to(DEV).train()
        opt = mrdis.ArenaAdam(model.parameters(), lr=1e-3, weight_decay=1e-5)
        st_np, st_t = np.random.get_state(), torch.get_rng_state()
        plans = list(la.batch_plan())
        np.random.set_state(st_np); torch.set_rng_state(st_t)
        out = losses[fed] = []
        for b, (_, _, metas) in list(zip(la, plans)):              # the epoch's batches are assembled before the first step draws anything
            x, t = (b['inputs'], b['targets']) if fed == 'loader' else _torch_batch(la.dataset.store, la.dataset, metas, 3)
            torch.manual_seed(20 + len(out))
            loss, _ = mrdis.nvnet_loss(*model(x), x, t)
            loss.backward()
            opt.step(fused_clip=True)
            opt.zero_grad()
            out.append(float(loss.detach()))
        assert len(out) == 2
    assert losses['loader'] == losses['torch'], losses
    assert losses['loader'][0] != losses['loader'][1] and all(np.isfinite(losses['loader']))


def test_gather_replays_through_a_graph_with_the_next_batch(mrdis):
    """every per-batch value comes from the device table, so a captured pair of launches replayed after the NEXT batch's table was copied into the same
    buffer gives that batch's inputs and targets (other subjects, masks, flips, scales)"""
    data = data3d_volumes()
    la = _loader(mrdis, data, True, K=3)
    ds, st = la.dataset, la.dataset.store
    H, W, D = st.shape
    z0, Dz = ds.crop()
    np.random.seed(21); torch.manual_seed(22)
    plans = [p for _ in range(2) for p in la.batch_plan() if len(p[2]) == 2]
    tabs = [torch.from_numpy(la.table(m)[0]).to(DEV) for _, _, m in plans]
    assert len(tabs) == 4 and not torch.equal(tabs[0], tabs[1])
    static = tabs[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        mrdis.hip.volume_gather(static, 4, H, W, D, z0, Dz)                     # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        x, mask = mrdis.hip.volume_gather(static, 4, H, W, D, z0, Dz)
        t = mrdis.hip.volume_gather(static, 4, H, W, D, z0, Dz, targets=True, K=3, relabel=True)
    for tab, (_, _, metas) in zip(tabs, plans):
        static.copy_(tab)
        g.replay()
        wx, wt = _torch_batch(st, ds, metas, 3)
        assert torch.equal(x, wx) and torch.equal(t, wt)
        assert mask.cpu().tolist() == la.table(metas)[1].tolist()
