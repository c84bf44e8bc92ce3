"""Missing-modality evaluation on the MI355X: the fused cosine top-1 search (csrc/mrdis_zsearch.hip, hip.cosine_top1) against a float64
restatement of the reference's compute_cosine + argmax (model.py:3396-3415), its edge cases and determinism, and EvalStep /
Run.evaluate with info = 'nearest_neighbour' | 'mean' (main_missing.py:374-430) end to end."""
import itertools
import os

import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def ref_cos64(G, Q):
    """compute_cosine in float64: norm = max(sqrt(sum x^2 + 1e-8), 1e-8); (Q, N)"""
    G, Q = G.double(), Q.double()
    gn = torch.clamp_min(torch.sqrt((G * G).sum(1) + 1e-8), 1e-8)
    qn = torch.clamp_min(torch.sqrt((Q * Q).sum(1) + 1e-8), 1e-8)
    return (Q @ G.t()) / (qn[:, None] * gn[None, :])


def check_top1(G, glab, Q, qlab, idx, cos):
    c64 = ref_cos64(G, Q)
    c64 = torch.where(glab[None, :].long() == qlab[:, None].long(), torch.full_like(c64, -float('inf')), c64)
    idx, cos = idx.long().cpu(), cos.cpu()
    c64 = c64.cpu()
    for q in range(Q.shape[0]):
        row = c64[q]
        if torch.isinf(row).all():
            assert idx[q] == -1 and cos[q] == -float('inf'), (q, int(idx[q]), float(cos[q]))
            continue
        top = row.max()
        i = int(idx[q])
        assert 0 <= i < G.shape[0] and not torch.isinf(row[i]), (q, i)
        assert float(top - row[i]) <= 2e-6, (q, i, float(top), float(row[i]))                 # a float64 top-1 within 2e-6
        assert abs(float(cos[q]) - float(row[i])) <= 2e-6, (q, float(cos[q]), float(row[i]))
        if row.numel() > 1:
            t2 = torch.topk(row, 2).values
            if float(t2[0] - t2[1]) > 1e-4:
                assert i == int(row.argmax()), (q, i, int(row.argmax()))


@pytest.mark.parametrize('N,D,Q', list(itertools.product([1, 63, 1000, 40000], [480, 1024, 37], [1, 32, 64])))
def test_cosine_top1_vs_float64(mrdis, N, D, Q):
    g = torch.Generator(device=DEV).manual_seed(N * 7 + D * 3 + Q)
    G = torch.randn(N, D, device=DEV, generator=g)
    Qm = torch.randn(Q, D, device=DEV, generator=g)
    Qm[: Q // 2] += 0.5 * G[torch.randint(0, N, (Q // 2,), device=DEV, generator=g)]          # half the queries near a gallery row
    glab = torch.randint(0, 5, (N,), device=DEV, generator=g, dtype=torch.int32)
    qlab = torch.randint(0, 5, (Q,), device=DEV, generator=g, dtype=torch.int32)
    before = mrdis.hip.launch_counts()['zsearch']
    idx, cos = mrdis.hip.cosine_top1(G, glab, Qm, qlab)
    assert mrdis.hip.launch_counts()['zsearch'] == before + 1
    check_top1(G, glab, Qm, qlab, idx, cos)


def test_exclusion_labels(mrdis):
    N, D, Q = 300, 480, 8
    G = torch.randn(N, D, device=DEV)
    Qm = torch.randn(Q, D, device=DEV)
    glab = torch.zeros(N, dtype=torch.int32, device=DEV)
    glab[137] = 1                                                                     # every row but one excluded
    idx, cos = mrdis.hip.cosine_top1(G, glab, Qm, torch.zeros(Q, dtype=torch.int32, device=DEV))
    assert (idx.cpu() == 137).all()
    check_top1(G, glab, Qm, torch.zeros(Q, dtype=torch.int32, device=DEV), idx, cos)
    idx, cos = mrdis.hip.cosine_top1(G, torch.full((N,), 4, dtype=torch.int32, device=DEV), Qm, torch.full((Q,), 4, dtype=torch.int32, device=DEV))
    assert (idx.cpu() == -1).all() and (cos.cpu() == -float('inf')).all()                # every row excluded


def test_duplicated_rows_give_the_smallest_index(mrdis):
    N, D = 5000, 1024
    G = torch.randn(N, D, device=DEV)
    Qm = torch.randn(4, D, device=DEV)
    for r in (4100, 17, 2999, 611):
        G[r] = Qm[0] * 3.0
    G[4999] = Qm[1]
    G[1] = Qm[1]
    lab = torch.zeros(N, dtype=torch.int32, device=DEV)
    idx, _ = mrdis.hip.cosine_top1(G, lab, Qm, torch.ones(4, dtype=torch.int32, device=DEV))
    assert int(idx[0]) == 17 and int(idx[1]) == 1


def test_zero_rows_give_cosine_zero(mrdis):
    N, D = 200, 480
    G = torch.zeros(N, D, device=DEV)
    Qm = torch.randn(3, D, device=DEV)
    Qm[2] = 0
    idx, cos = mrdis.hip.cosine_top1(G, torch.zeros(N, dtype=torch.int32, device=DEV), Qm, torch.ones(3, dtype=torch.int32, device=DEV))
    assert (cos.cpu() == 0).all() and (idx.cpu() == 0).all()                            # 0 / (1e-4 * norm): through the 1e-8 clamps


@pytest.mark.parametrize('ld_extra', [5, 480])
def test_gallery_row_stride(mrdis, ld_extra):
    N, D, Q = 3000, 480, 32
    wide = torch.randn(N, D + ld_extra, device=DEV)
    G = wide[:, :D]
    assert G.stride(0) == D + ld_extra
    Qm = torch.randn(Q, D, device=DEV)
    Qm[:8] += G[100:108]
    glab = torch.randint(0, 3, (N,), dtype=torch.int32, device=DEV)
    qlab = torch.randint(0, 3, (Q,), dtype=torch.int32, device=DEV)
    idx, cos = mrdis.hip.cosine_top1(G, glab, Qm, qlab)
    check_top1(G.contiguous(), glab, Qm, qlab, idx, cos)
    idx2, cos2 = mrdis.hip.cosine_top1(G.contiguous(), glab, Qm, qlab)
    assert torch.equal(idx, idx2)


def test_bit_identical_across_launches_and_grid_sizes(mrdis):
    N, D, Q = 40000, 1024, 64
    G = torch.randn(N, D, device=DEV)
    Qm = torch.randn(Q, D, device=DEV)
    glab = torch.randint(0, 9, (N,), dtype=torch.int32, device=DEV)
    qlab = torch.randint(0, 9, (Q,), dtype=torch.int32, device=DEV)
    a = mrdis.hip.cosine_top1(G, glab, Qm, qlab)
    b = mrdis.hip.cosine_top1(G, glab, Qm, qlab)
    outs = []
    for grid in (1, 37, 2048):
        with mrdis.hip.option('zsearch_grid', grid):
            outs.append(mrdis.hip.cosine_top1(G, glab, Qm, qlab))
    for o in [b] + outs:
        assert torch.equal(a[0], o[0]) and torch.equal(a[1].view(torch.int32), o[1].view(torch.int32))


# --------------------------------------------------------------------------- end to end: EvalStep / Run.evaluate
M, B, H, W = 4, 4, 160, 192


@pytest.fixture(scope='module')
def setup(mrdis):
    cfg = dict(mrdis.DEFAULT_CONFIG)
    cfg.update(contrast_list=[f'm{i}' for i in range(M)], input_height=H, input_width=W, batch_size=B)
    cfg = mrdis.derive_config(cfg, DEV)
    torch.manual_seed(3); np.random.seed(3)
    model = mrdis.build_model(cfg)
    x, mask, mask_img = mrdis.synthetic_batch(B, M, H, W, seed=4)
    args = (x.to(DEV).contiguous(memory_format=torch.channels_last), mask.to(DEV), mask_img.to(DEV), mask)
    plain = mrdis.EvalStep(model, cfg)
    torch.manual_seed(5); np.random.seed(5)
    out0 = plain(*args)
    # the query's compact anatomy codes; a gallery of random positive codes (cosines to the query ~0.8) with, for every query b and
    # source contrast, its own code planted at one row of ANOTHER subject (cosine 1) and, at a smaller index, at one row of ITS OWN subject
    comp = [model.compute_compact_s(s) for s in out0[3]['si_list']]
    Dc = comp[0].shape[1]
    N, S = 600, 6
    gen = torch.Generator(device=DEV).manual_seed(9)
    s_c = torch.rand(N, M, Dc, device=DEV, generator=gen)
    z = torch.randn(N, M, cfg['z_size'], device=DEV, generator=gen)
    subject = (torch.arange(N, device=DEV) // (N // S)).to(torch.int32)
    subj_id = [f'S{k}' for k in (0, 0, 2, 5)]                                  # two slices of one subject in the batch
    codes = [0, 0, 2, 5]
    want = {}
    for src in sorted({mrdis.nn_source_contrast(i) for i in range(M)}):
        for b in range(B):
            own = codes[b] * (N // S) + 3 + 10 * src + b
            other = ((codes[b] + 1 + b) % S) * (N // S) + 40 + 10 * src + b
            s_c[own, src] = comp[src][b]
            s_c[other, src] = comp[src][b]
            want[(src, b)] = other
    gal = mrdis.ZGallery(s_c, z, subject, torch.arange(N, device=DEV), [f'S{k}' for k in range(S)])
    return dict(cfg=cfg, model=model, args=args, out0=out0, gal=gal, subj_id=subj_id, want=want)


def test_nearest_neighbour_eval_step(mrdis, setup):
    cfg, model, args, gal, want = setup['cfg'], setup['model'], setup['args'], setup['gal'], setup['want']
    step = mrdis.EvalStep(model, cfg, info='nearest_neighbour', gallery=gal)
    mrdis.hip.launch_counts(reset=True)
    torch.manual_seed(5); np.random.seed(5)
    loss, parts, metrics, aux = step(*args, subj_id=setup['subj_id'])
    assert mrdis.hip.launch_counts()['zsearch'] == 3                                  # distinct source contrasts of M = 4: {1, 0, 2}
    # a CPU torch search over the same gallery (float32 compute_cosine, own subject excluded); z rows are distinct, so z_find names its row
    codes = gal.codes(setup['subj_id'])
    excl = gal.subject.cpu()[None, :].long() == torch.tensor(codes)[:, None]
    for i in range(M):
        src = mrdis.nn_source_contrast(i)
        q = model.compute_compact_s(aux['si_list'][src]).cpu()
        G = gal.s_compact[:, src].cpu()
        cs = (q @ G.t()) / (torch.clamp_min(torch.sqrt((q * q).sum(1) + 1e-8), 1e-8)[:, None] * torch.clamp_min(torch.sqrt((G * G).sum(1) + 1e-8), 1e-8)[None])
        cs = torch.where(excl, torch.full_like(cs, -float('inf')), cs)
        pick = cs.argmax(1)
        c64 = torch.where(excl, torch.full_like(cs, -float('inf'), dtype=torch.float64), ref_cos64(G, q))
        for b in range(B):
            got = int((gal.z[:, i] - aux['z_find'][i][b]).abs().sum(1).argmin())
            assert torch.equal(aux['z_find'][i][b], gal.z[got, i]), (i, b)
            assert int(gal.subject[got]) != codes[b]                                     # own-subject rows never picked
            assert float(c64[b].max() - c64[b, got]) <= 2e-6, (i, b)
            top2 = torch.topk(c64[b], 2).values
            if float(top2[0] - top2[1]) > 1e-4:
                assert got == int(pick[b]), (i, b, got, int(pick[b]))
            assert float(c64[b, want[(src, b)]]) >= float(c64[b].max()) - 1e-6          # the planted row is a top-1
    # the two reconstructions are the model's, decoded with z_find; the plain pass's own codes still feed sim_z / latent_z
    with torch.no_grad():
        model.eval()
        try:
            xi = model.reconstruct_input_si_zi(aux['si_list'], aux['z_find'])
            xm = model.reconstruct_input_si_zj(aux['si_list'], aux['z_find'])
        finally:
            model.train()
    for a, b in zip(xi + xm, aux['xi_fake_list'] + aux['xi_fake_mix_list']):
        assert float((a - b).abs().max()) <= 1e-6
    for a, b in zip(aux['zi_list'], setup['out0'][3]['zi_list']):
        assert torch.equal(a, b)
    assert torch.isfinite(loss) and set(metrics) == {'rmse', 'psnr', 'ssim'}


def test_mean_eval_step(mrdis, setup):
    cfg, model, args, gal = setup['cfg'], setup['model'], setup['args'], setup['gal']
    step = mrdis.EvalStep(model, cfg, info='mean', gallery=gal)
    mrdis.hip.launch_counts(reset=True)
    _, _, _, aux = step(*args, subj_id=setup['subj_id'])
    assert mrdis.hip.launch_counts()['zsearch'] == 0
    codes = gal.codes(setup['subj_id'])
    for i in range(M):
        for b in range(B):
            keep = gal.subject != codes[b]
            want = gal.z[keep, i].mean(0)                                              # compute_mean_z_by_s
            assert float((aux['z_find'][i][b] - want).abs().max()) <= 1e-6, (i, b)


def test_plain_eval_step_is_unchanged(mrdis, setup):
    cfg, model, args = setup['cfg'], setup['model'], setup['args']
    torch.manual_seed(5); np.random.seed(5)
    loss, parts, metrics, aux = mrdis.EvalStep(model, cfg, info='')(*args)
    l0, p0, m0, a0 = setup['out0']
    assert torch.equal(loss, l0) and 'z_find' not in aux
    for k in p0:
        assert torch.equal(parts[k], p0[k]), k
    for k in m0:
        assert torch.equal(metrics[k], m0[k]), k
    for a, b in zip(aux['xi_fake_mix_list'], a0['xi_fake_mix_list']):
        assert torch.equal(a, b)


def test_build_gallery_round_trip_and_entry_point(mrdis, tmp_path, monkeypatch):
    """Run.evaluate(info='nearest_neighbour') through main() with `eval_info` on a tiny synthetic set: the gallery is built by one encoder pass,
    saved under ckpt_path/result_test/, reloaded bit for bit, and the usual stat keys come back."""
    store = mrdis.train.synthetic_store
    monkeypatch.setattr(mrdis.train, 'synthetic_store', lambda config, device: store(config, device, n_subj=10))      # a test split of two subjects
    base = dict(contrast_list=['T1', 'T2'], input_height=64, input_width=64, batch_size=4, epochs=1, gpu='0', data_source='synthetic',
                ckpt_root=str(tmp_path / 'ckpt'), ckpt_timelabel='t0', shuffle=False)
    (tmp_path / 'train.yaml').write_text(yaml.dump(base))
    cfg = mrdis.train.setup_config(str(tmp_path / 'train.yaml'), device=DEV)
    run = mrdis.train.Run(cfg, log=lambda *a: None)
    run.train(max_iters_per_epoch=2)
    gal = mrdis.build_z_gallery(run, run.loaders['test'])
    assert gal.s_compact.shape[1:] == (2, 4 * (64 // 16) * (64 // 16)) and gal.z.shape[1:] == (2, cfg['z_size'])
    assert len(gal) == len(run.loaders['test'].dataset) and len(gal.subjects) >= 2
    p = gal.save(str(tmp_path / 'g.pt'))
    back = mrdis.ZGallery.load(p, DEV)
    for k in ('s_compact', 'z', 'subject', 'slice_idx'):
        assert torch.equal(getattr(gal, k), getattr(back, k)), k
    assert back.subjects == gal.subjects
    for info in ('nearest_neighbour', 'mean'):
        (tmp_path / 'test.yaml').write_text(yaml.dump({**base, 'phase': 'test', 'eval_info': info, 'ckpt_name': 'epoch000.pth.tar',
                                                       'ckpt_timelabel': os.path.basename(cfg['ckpt_path'])}))     # a training run names its directory by the clock
        mrdis.hip.launch_counts(reset=True)
        r = mrdis.train.main([str(tmp_path / 'test.yaml')])
        assert os.path.exists(r.z_gallery_path('test'))
        if info == 'nearest_neighbour':
            assert mrdis.hip.launch_counts()['zsearch'] >= 2
        stat = r.evaluate(phase='test', set_='test', info=info)
        assert {'rmse', 'psnr', 'ssim', 'recon_x_mix', 'all'} <= set(stat) and np.isfinite(stat['all'])
    saved = mrdis.ZGallery.load(r.z_gallery_path('test'), DEV)
    assert torch.equal(saved.subject, gal.subject) and saved.subjects == gal.subjects
    for k in ('s_compact', 'z'):                                               # same weights (the epoch-0 checkpoint), same set, same encoder pass
        assert torch.allclose(getattr(saved, k), getattr(gal, k), rtol=0, atol=1e-6), k
