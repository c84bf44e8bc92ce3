"""Whole-subject synthesis of missing contrasts on the MI355X (phase: synthesize): the two assembly kernels of csrc/mrdis_synth.hip against a
float64 CPU restatement of the rules (synth.py's docstring: this package's own convention), and `synthesize_volumes` / `Run.synthesize` /
the entry point end to end on the smallest model (M = 3, 32 x 32) over a 12-slice store with one incomplete subject.

Tolerance of every accumulated value: measured here, not fixed.  The fp32 torch composition that adds the same values in the same order is
compared with the float64 sum; the kernel may be at most twice as far off (the factor covers a different contraction of the adds).  Counts,
the division, the transpose and the fill are exact."""
import os

import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


# --------------------------------------------------------------------------- the rules, on the CPU
def contributions(D, b, c_lo, c_hi, launches):
    """per plane k the ordered list of (launch, sample r, channel c): launch order, then r ascending"""
    out = [[] for _ in range(D)]
    for li, (s0, B) in enumerate(launches):
        for k in range(D):
            for r in range(B):
                c = k - (s0 + r) + b
                if c_lo <= c <= c_hi:
                    out[k].append((li, r, c))
    return out


def assemble(recons, launches, D, b, c_lo, c_hi, dtype):
    """recons[launch][source] (B, C, H, W) CPU tensors -> (acc (D, H, W) of `dtype` summed in the kernel's order, cnt (D,) int32)"""
    H, W = recons[0][0].shape[2:]
    acc = torch.zeros(D, H, W, dtype=dtype)
    cnt = torch.zeros(D, dtype=torch.int32)
    for k, lst in enumerate(contributions(D, b, c_lo, c_hi, launches)):
        for li, r, c in lst:
            for x in recons[li]:
                acc[k] += x[r, c].to(dtype)
                cnt[k] += 1
    return acc, cnt


def check_close(tag, got, ref32, ref64):
    """the measured bound: |kernel - float64| <= 2 max|fp32 composition - float64|"""
    kerr = float((got.double() - ref64).abs().max())
    terr = float((ref32.double() - ref64).abs().max())
    print(f'[synth {tag}] max |x - float64|: kernel {kerr:.3e}  torch fp32 composition {terr:.3e}  (max |x| {float(ref64.abs().max()):.2f})')
    assert kerr <= 2 * terr, (tag, kerr, terr)


def cl(x):
    return x.contiguous(memory_format=torch.channels_last)


def make_recons(launches, n_src, C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return [[cl(torch.randn(B, C, H, W, generator=g)) for _ in range(n_src)] for _, B in launches]


def run_accum(mrdis, recons, launches, D, c_lo, c_hi):
    H, W = recons[0][0].shape[2:]
    acc = torch.zeros(D, H, W, device=DEV)
    cnt = torch.zeros(D, dtype=torch.int32, device=DEV)
    for (s0, B), srcs in zip(launches, recons):
        mrdis.hip.synth_accum([cl(x.to(DEV)) for x in srcs], range(s0, s0 + B), acc, cnt, c_lo, c_hi)
    return acc, cnt


# --------------------------------------------------------------------------- kernels
ACCUM_CASES = {
    # name: (C, H, W, D, launches [(s0, B)], sources, mean mode)
    'centre1': (7, 5, 6, 12, [(3, 4)], 1, False),
    'mean3': (7, 5, 6, 12, [(3, 4), (7, 2)], 3, True),
    'aligned': (3, 8, 16, 9, [(1, 5), (6, 2)], 2, True),                  # H W % 4 == 0: 16 bytes of acc per lane
    'aligned_centre': (3, 8, 16, 9, [(1, 5), (6, 2)], 2, False),
    'c1': (1, 5, 6, 5, [(0, 3), (3, 2)], 2, True),                        # b = 0
    'tiles4': (3, 40, 52, 6, [(1, 4)], 2, True),                          # 2080 pixels: three 1024-pixel vector tiles, the last ragged
    'tiles1': (3, 33, 35, 6, [(1, 4)], 8, True),                          # 1155 pixels, not a multiple of 4: five 256-pixel tiles; eight sources
    'guard': (3, 5, 6, 4, [(0, 4)], 2, True),                             # centres 0 .. 3 of a 4-plane volume predict planes -1 and 4: dropped
}


@pytest.mark.parametrize('name', list(ACCUM_CASES))
def test_accum_vs_float64(mrdis, name):
    C, H, W, D, launches, n_src, mean = ACCUM_CASES[name]
    b = (C - 1) // 2
    c_lo, c_hi = (0, 2 * b) if mean else (b, b)
    recons = make_recons(launches, n_src, C, H, W, seed=len(name) * 31 + C)
    before = mrdis.hip.launch_counts()
    acc, cnt = run_accum(mrdis, recons, launches, D, c_lo, c_hi)
    after = mrdis.hip.launch_counts()
    assert after['synthaccum'] == before['synthaccum'] + len(launches) and after['synthfinish'] == before['synthfinish']
    ref64, cnt64 = assemble(recons, launches, D, b, c_lo, c_hi, torch.float64)
    ref32, _ = assemble(recons, launches, D, b, c_lo, c_hi, torch.float32)
    assert torch.equal(cnt.cpu(), cnt64), (cnt.cpu().tolist(), cnt64.tolist())
    check_close(f'accum {name}', acc.cpu(), ref32, ref64)
    acc2, cnt2 = run_accum(mrdis, recons, launches, D, c_lo, c_hi)                      # two runs, the same bits
    assert torch.equal(acc.view(torch.int32), acc2.view(torch.int32)) and torch.equal(cnt, cnt2)
    if name == 'centre1':
        assert cnt64.tolist() == [0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 0, 0]
        for r in range(4):
            assert torch.equal(acc[3 + r].cpu(), recons[0][0][r, 3])                    # the input channel, bit for bit
        assert not acc[:3].any() and not acc[7:].any()
    if name == 'mean3':
        assert (cnt64 > 0).all() and len(set(cnt64.tolist())) > 2                       # every plane covered, with varying counts
        first = contributions(D, b, c_lo, c_hi, launches[:1])
        second = contributions(D, b, c_lo, c_hi, [(0, 0)] + launches[1:])
        assert [k for k in range(D) if first[k] and second[k]] == [4, 5, 6, 7, 8, 9]      # planes fed by both launches
    if name == 'guard':
        assert cnt64.tolist() == [4, 6, 6, 4]


def test_accum_adds_to_what_is_there(mrdis):
    """acc and cnt are read-modify-write: a second target's launches must not disturb planes they do not cover"""
    C, H, W, D = 3, 8, 16, 9
    x = make_recons([(3, 2)], 1, C, H, W, seed=5)
    acc = torch.full((D, H, W), 0.5, device=DEV)
    cnt = torch.arange(D, dtype=torch.int32, device=DEV)
    mrdis.hip.synth_accum([x[0][0].to(DEV)], [3, 4], acc, cnt, 1, 1)
    assert cnt.cpu().tolist() == [0, 1, 2, 4, 5, 5, 6, 7, 8]
    want = torch.full((D, H, W), 0.5)
    want[3] += x[0][0][0, 1]; want[4] += x[0][0][1, 1]
    assert torch.equal(acc.cpu(), want)


@pytest.mark.parametrize('D,H,W', [(12, 5, 6), (37, 5, 6), (16, 8, 32), (170, 3, 7)], ids=str)      # 170: two chunks of planes per pixel tile
@pytest.mark.parametrize('fill', [-10.0, 0.3])
def test_finish_is_exact(mrdis, D, H, W, fill):
    g = torch.Generator().manual_seed(D * 7 + W)
    acc = torch.randn(D, H, W, generator=g) * 5
    cnt = torch.randint(1, 22, (D,), generator=g, dtype=torch.int32)
    cnt[1] = 0; cnt[D - 2] = 0
    want = acc / cnt.float()[:, None, None]                                              # IEEE fp32 division on the CPU
    f32 = torch.tensor(fill, dtype=torch.float32)
    want[cnt == 0] = f32
    before = mrdis.hip.launch_counts()
    a = acc.to(DEV)
    vol, out = mrdis.hip.synth_finish(a, cnt.to(DEV), fill)
    after = mrdis.hip.launch_counts()
    assert after['synthfinish'] == before['synthfinish'] + 1 and after['synthaccum'] == before['synthaccum']
    assert vol.data_ptr() == a.data_ptr() and tuple(out.shape) == (H, W, D) and out.is_contiguous()
    assert torch.equal(vol.cpu().view(torch.int32), want.view(torch.int32))              # bit-equal quotient, in place
    assert torch.equal(out.cpu().view(torch.int32), want.permute(1, 2, 0).contiguous().view(torch.int32))
    assert (vol[1] == f32.item()).all() and (vol[D - 2] == f32.item()).all()
    vol2, out2 = mrdis.hip.synth_finish(acc.to(DEV), cnt.to(DEV), fill)
    assert torch.equal(out.view(torch.int32), out2.view(torch.int32)) and torch.equal(vol.view(torch.int32), vol2.view(torch.int32))


def test_wrappers_refuse_other_layouts(mrdis):
    acc = torch.zeros(12, 5, 6, device=DEV)
    cnt = torch.zeros(12, dtype=torch.int32, device=DEV)
    x = cl(torch.zeros(4, 7, 5, 6, device=DEV))
    before = mrdis.hip.launch_counts()
    for bad in (lambda: mrdis.hip.synth_accum([x.contiguous()], range(3, 7), acc, cnt, 3, 3),
                lambda: mrdis.hip.synth_accum([x], [3, 4, 5, 7], acc, cnt, 3, 3),
                lambda: mrdis.hip.synth_accum([x], range(3, 7), acc.permute(0, 2, 1), cnt, 3, 3),
                lambda: mrdis.hip.synth_accum([x], range(3, 7), acc, cnt.long(), 3, 3),
                lambda: mrdis.hip.synth_accum([x, x.half()], range(3, 7), acc, cnt, 3, 3),
                lambda: mrdis.hip.synth_accum([x], range(3, 7), acc, cnt, 3, 7),
                lambda: mrdis.hip.synth_finish(acc.permute(1, 0, 2), cnt),
                lambda: mrdis.hip.synth_finish(acc, cnt[:5])):
        with pytest.raises(mrdis.MrdisError):
            bad()
    assert mrdis.hip.launch_counts() == before


# --------------------------------------------------------------------------- end to end
M, H, W, D, BS, BLK = 3, 32, 32, 12, 4, 3
NAMES = ['c0', 'c1', 'c2']
SUBJ = ['S0', 'S1', 'S2', 'S3']                                                       # S3 lacks c0 and c1


def decode_batches(mrdis, st, sid, present, z_of=None):
    """the oracle's half of the driver: the same batches through the same model calls -> per batch the CPU fp32 `reconstruct_input_si_zj`
    outputs as {(source, target): (B, C, H, W)} and the encodings.  z_of(i, si_list, mu_list, B): the code of an absent target i."""
    model, cfg, store = st['model'], st['cfg'], st['store']
    outs = []
    was = model.training
    model.eval()
    try:
        with torch.no_grad(), mrdis.ops.mix_cache():
            for s0, B in mrdis.synth_plan(D, BLK, BS):
                ptrs = torch.tensor([[store.ptr(f'{sid}/{c}') if present[i] else 0 for i, c in enumerate(NAMES)]] * B, dtype=torch.int64).to(DEV)
                idx = torch.arange(s0, s0 + B, dtype=torch.int32).to(DEV)
                none = torch.full((B,), -1, dtype=torch.int32).to(DEV)
                inputs, _, mask_img = mrdis.hip.slice_gather(ptrs, idx, none, H, W, D, BLK)
                si, mu = mrdis.trainer._encode_batch(model, cfg, inputs, mask_img)
                z = list(mu)
                for i in range(M):
                    if not present[i] and z_of is not None:
                        z[i] = z_of(i, si, mu, B)
                mix = model.reconstruct_input_si_zj(si, z)
                pairs = [(j, i) for j in range(M) for i in range(M) if i != j]
                outs.append({p: x.float().cpu() for p, x in zip(pairs, mix)})
    finally:
        model.train(was)
    return outs


def check_volume(tag, mrdis, vol_hwd, outs, target, sources, mean, fill=-10.0):
    """vol_hwd (H, W, D) from the driver against the float64 / fp32 fuse of the oracle's decodes"""
    launches = mrdis.synth_plan(D, BLK, BS)
    c_lo, c_hi = (0, 2 * BLK) if mean else (BLK, BLK)
    recons = [[o[(j, target)] for j in sources] for o in outs]
    acc64, cnt = assemble(recons, launches, D, BLK, c_lo, c_hi, torch.float64)
    acc32, _ = assemble(recons, launches, D, BLK, c_lo, c_hi, torch.float32)
    cov = cnt > 0
    ref64 = acc64[cov] / cnt[cov].double()[:, None, None]
    ref32 = acc32[cov] / cnt[cov].float()[:, None, None]
    got = vol_hwd.cpu().permute(2, 0, 1)
    check_close(tag, got[cov], ref32, ref64)
    assert (got[~cov] == fill).all()
    return cov


@pytest.fixture(scope='module')
def st(mrdis):
    cfg = dict(mrdis.DEFAULT_CONFIG)
    cfg.update(contrast_list=NAMES, input_height=H, input_width=W, batch_size=BS, block_size=BLK)
    cfg = mrdis.derive_config(cfg, DEV)
    torch.manual_seed(3); np.random.seed(3)
    model = mrdis.build_model(cfg)
    g = np.random.RandomState(17)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    inside = (((yy - H / 2 + 0.5) / (0.40 * H)) ** 2 + ((xx - W / 2 + 0.5) / (0.42 * W)) ** 2) <= 1
    arrays = {}
    for s in SUBJ:
        for c in NAMES:
            v = np.where(inside[:, :, None], g.randn(H, W, D).astype(np.float32), np.float32(-10.0))
            if not (s == 'S3' and c in ('c0', 'c1')):
                arrays[f'{s}/{c}'] = v
    store = mrdis.VolumeStore.from_arrays(arrays, DEV)
    subj = [s for s in SUBJ for _ in range(BLK, D - BLK)]
    idx = [k for _ in SUBJ for k in range(BLK, D - BLK)]
    ds = mrdis.SliceDataset('BraTS', store, subj, idx, block_size=BLK, contrast_list=NAMES)
    gallery = mrdis.build_z_gallery(model, mrdis.BatchLoader(ds, BS), cfg)
    out = dict(cfg=cfg, model=model, store=store, arrays=arrays, gallery=gallery)
    out['full'] = decode_batches(mrdis, out, 'S0', [True] * M)                           # computed once, shared by the tests below
    return out


def test_complete_subject_centre(mrdis, st):
    model = st['model'].train()
    mrdis.hip.launch_counts(reset=True)
    res = list(mrdis.synthesize_volumes(model, st['cfg'], st['store'], ['S0']))
    cnt = mrdis.hip.launch_counts()
    assert cnt['synthaccum'] == 2 * M and cnt['synthfinish'] == M and cnt['zsearch'] == 0      # two batches x three targets
    assert model.training                                                                # the flag is restored
    assert len(res) == 1
    res = res[0]
    assert res['subj_id'] == 'S0' and res['present'] == [True] * M and res['dropped'] == [False] * M
    assert res['targets'] == [0, 1, 2] and res['skipped'] == [] and res['n_sources'] == {c: 2 for c in NAMES}
    for i, c in enumerate(NAMES):
        v = res['volumes'][c]
        assert tuple(v.shape) == (H, W, D) and v.dtype == torch.float32 and v.is_contiguous()
        cov = check_volume(f'S0 {c} centre', mrdis, v, st['full'], i, [j for j in range(M) if j != i], mean=False)
        assert cov.tolist() == [BLK <= k <= D - 1 - BLK for k in range(D)]
        assert all(np.isfinite(x) for x in res['metrics'][c])
        # the score: recon_metrics of the covered planes against the store, averaged
        truth = st['store'].vols[f'S0/{c}'][BLK:D - BLK].unsqueeze(1)
        want = mrdis.hip.recon_metrics(truth, v.permute(2, 0, 1)[BLK:D - BLK].unsqueeze(1).contiguous()).double().mean(0).cpu()
        # (the same kernel on the same planes, through a copy instead of a view: fp32 outputs, so a few units of 2^-24 at the most)
        assert torch.allclose(torch.tensor(res['metrics'][c], dtype=torch.float64), want, rtol=1e-6, atol=0), (c, res['metrics'][c], want)
    again = next(mrdis.synthesize_volumes(model, st['cfg'], st['store'], ['S0']))
    for c in NAMES:
        assert torch.equal(res['volumes'][c].view(torch.int32), again['volumes'][c].view(torch.int32))


def test_block_mean(mrdis, st):
    centre = next(mrdis.synthesize_volumes(st['model'], st['cfg'], st['store'], ['S0']))
    res = next(mrdis.synthesize_volumes(st['model'], st['cfg'], st['store'], ['S0'], block='mean'))
    for i, c in enumerate(NAMES):
        cov = check_volume(f'S0 {c} mean', mrdis, res['volumes'][c], st['full'], i, [j for j in range(M) if j != i], mean=True)
        assert cov.all()                                                                 # every plane is predicted by some block
        assert not torch.equal(res['volumes'][c][:, :, BLK:D - BLK], centre['volumes'][c][:, :, BLK:D - BLK])
        assert all(np.isfinite(x) for x in res['metrics'][c])


def test_dropped_contrast_nearest_neighbour(mrdis, st):
    gal = st['gallery']
    code = gal.codes(['S0'])[0]
    assert code >= 0
    mrdis.hip.launch_counts(reset=True)
    res = next(mrdis.synthesize_volumes(st['model'], st['cfg'], st['store'], ['S0'], info='nearest_neighbour', gallery=gal, drop=['c1']))
    assert mrdis.hip.launch_counts()['zsearch'] == 2                                     # one search per batch: source contrast 0
    assert res['present'] == [True, False, True] and res['dropped'] == [False, True, False] and res['targets'] == [0, 1, 2]
    assert res['n_sources'] == {'c0': 1, 'c1': 2, 'c2': 1}
    assert all(np.isfinite(x) for x in res['metrics']['c1'])                             # scored against the hidden truth
    rows = res['nn_rows']['c1'].cpu()
    assert set(res['nn_rows']) == {'c1'} and rows.numel() == D - 2 * BLK
    assert (gal.subject.cpu()[rows] != code).all()                                       # never the subject's own rows
    seen = []

    def z_of(i, si, mu, B):
        assert i == 1 and mrdis.synth_source(1, [True, False, True]) == 0
        r = gal.nearest(st['model'].compute_compact_s(si[0]), [code] * B, 0).long()
        seen.append(r.cpu())
        return gal.z[r, 1]
    outs = decode_batches(mrdis, st, 'S0', [True, False, True], z_of)
    assert torch.equal(torch.cat(seen), rows)                                            # the code is gallery.z[gallery.nearest(...), 1]
    # S0's own rows hold the very same anatomy code (cosine 1): without the exclusion they would win
    own = gal.nearest(gal.s_compact[gal.subject == code][:, 0].contiguous(), [-1] * int((gal.subject == code).sum()), 0).cpu()
    assert (gal.subject.cpu()[own.long()] == code).all()
    check_volume('S0 c1 dropped, nearest neighbour', mrdis, res['volumes']['c1'], outs, 1, [0, 2], mean=False)
    check_volume('S0 c0 with c1 dropped', mrdis, res['volumes']['c0'], outs, 0, [2], mean=False)


def test_incomplete_subject(mrdis, st):
    gal = st['gallery']
    res = next(mrdis.synthesize_volumes(st['model'], st['cfg'], st['store'], ['S3'], info='mean', gallery=gal))
    assert res['present'] == [False, False, True] and res['dropped'] == [False] * M
    assert res['targets'] == [0, 1] and res['skipped'] == [2] and res['n_sources'] == {'c0': 1, 'c1': 1}
    code = gal.codes(['S3'])
    outs = decode_batches(mrdis, st, 'S3', [False, False, True], lambda i, si, mu, B: gal.mean_z(code * B, i).to(DEV))
    for i in (0, 1):
        assert all(np.isnan(x) for x in res['metrics'][NAMES[i]])                        # nothing to score against
        check_volume(f'S3 {NAMES[i]} from c2 alone', mrdis, res['volumes'][NAMES[i]], outs, i, [2], mean=False)
    plain = next(mrdis.synthesize_volumes(st['model'], st['cfg'], st['store'], ['S3']))
    assert plain['targets'] == [] and plain['skipped'] == [0, 1, 2] and plain['volumes'] == {}
    with pytest.raises(ValueError, match='no present contrast'):
        next(mrdis.synthesize_volumes(st['model'], st['cfg'], st['store'], ['S3'], drop=['c2']))
    nn = next(mrdis.synthesize_volumes(st['model'], st['cfg'], st['store'], ['S3'], info='nearest_neighbour', gallery=gal, fill=0.25))
    assert nn['targets'] == [0, 1] and set(nn['nn_rows']) == {'c0', 'c1'}
    assert (gal.subject.cpu()[nn['nn_rows']['c0'].cpu()] != code[0]).all()
    assert (nn['volumes']['c0'][:, :, :BLK] == 0.25).all() and (nn['volumes']['c0'][:, :, D - BLK:] == 0.25).all()


def test_entry_point_phase_synthesize(mrdis, tmp_path, monkeypatch):
    """train two iterations on the synthetic set, then phase=synthesize through main(): the .npy volumes and synth.csv appear under
    result_test/, and phase=test of the same checkpoint gives the same numbers before and after"""
    store = mrdis.train.synthetic_store
    monkeypatch.setattr(mrdis.train, 'synthetic_store', lambda config, device: store(config, device, n_subj=10))      # a test split of two subjects
    names = ['T1', 'T1c', 'T2']
    base = dict(contrast_list=names, input_height=H, input_width=W, batch_size=4, epochs=1, gpu='0', data_source='synthetic',
                ckpt_root=str(tmp_path / 'ckpt'), ckpt_timelabel='t0', shuffle=False)
    (tmp_path / 'train.yaml').write_text(yaml.dump(base))
    cfg = mrdis.train.setup_config(str(tmp_path / 'train.yaml'), device=DEV)
    mrdis.train.Run(cfg, log=lambda *a: None).train(max_iters_per_epoch=2)
    label = os.path.basename(cfg['ckpt_path'])
    later = {**base, 'ckpt_name': 'epoch000.pth.tar', 'ckpt_timelabel': label}

    def test_stat():
        (tmp_path / 'test.yaml').write_text(yaml.dump({**later, 'phase': 'test'}))
        return mrdis.train.main([str(tmp_path / 'test.yaml')]).evaluate(phase='test', set_='test')
    stat0 = test_stat()
    ckpt = open(os.path.join(cfg['ckpt_path'], 'epoch000.pth.tar'), 'rb').read()
    (tmp_path / 'synth.yaml').write_text(yaml.dump({**later, 'phase': 'synthesize', 'synth_info': 'nearest_neighbour', 'synth_drop': ['T1c']}))
    mrdis.hip.launch_counts(reset=True)
    run = mrdis.train.main([str(tmp_path / 'synth.yaml')])
    cnt = mrdis.hip.launch_counts()
    out_dir = os.path.join(run.config['ckpt_path'], 'result_test')
    ds = run.loaders['test'].dataset
    subjects = list(dict.fromkeys(str(s) for s in ds.subj_list))
    Hs, Ws, Ds = ds.store.shape
    assert len(subjects) == 2 and cnt['synthfinish'] == 2 * 3 and cnt['synthaccum'] == 2 * 3 * len(mrdis.synth_plan(Ds, BLK, 4)) and cnt['zsearch'] > 0
    for s in subjects:
        for c in names:
            v = np.load(os.path.join(out_dir, 'synth', f'{s}_{c}.npy'))
            assert v.shape == (Hs, Ws, Ds) and v.dtype == np.float32 and np.isfinite(v).all()
            assert (v[:, :, :BLK] == -10.0).all() and (v[:, :, BLK:Ds - BLK] != -10.0).any()
    lines = open(os.path.join(out_dir, 'synth.csv')).read().splitlines()
    assert lines[0] == 'subj_id,contrast,present,dropped,n_sources,mse,psnr,ssim' and len(lines) == 1 + 2 * 3
    for k, line in enumerate(lines[1:]):
        f = line.split(',')
        assert f[0] == subjects[k // 3] and f[1] == names[k % 3]
        assert (f[2], f[3], f[4]) == (('0', '1', '2') if f[1] == 'T1c' else ('1', '0', '1'))
        assert all(np.isfinite(float(x)) for x in f[5:])
    assert os.path.exists(run.z_gallery_path('test'))
    assert open(os.path.join(cfg['ckpt_path'], 'epoch000.pth.tar'), 'rb').read() == ckpt
    stat1 = test_stat()
    assert sorted(stat0) == sorted(stat1)
    assert np.array_equal(np.array([stat0[k] for k in sorted(stat0)]), np.array([stat1[k] for k in sorted(stat0)]), equal_nan=True), (stat0, stat1)
