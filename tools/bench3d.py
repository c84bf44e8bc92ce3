"""3-D path timing (BASELINE.json configs[4]: synthetic 4x128x128x128 volumes, batch 4, 1 GPU): one NVNet3D training
step (forward, nvnet_loss, backward, Adam on the flat arena) and, with --layers, every distinct Conv3d geometry of the
net (forward / data gradient / weight gradient, TFLOP/s against the 157 TFLOP/s fp32 MFMA peak).

    python tools/bench3d.py [--size 128] [--batch 4] [--channels 16] [--steps 5] [--layers]
    python tools/bench3d.py --loader [--batch 4] [--vol 160 192 155]      # the HBM-resident 3-D loader (data3d.py) in front of that step
    python tools/bench3d.py --loss-only                                   # the objective alone, forward + backward: torch composition vs fused HIP kernels
    python tools/bench3d.py --fused-loss                                  # the step with the torch objective and with the fused one, alternating windows
    python tools/bench3d.py --predict [--batch 4] [--vol 160 192 155]     # whole-volume sliding-window prediction: the two kernels, the torch composition, a batch end to end

--loader builds a synthetic BraTS-shaped store, times the one-launch batch gather (mrdis_volume_gather) beside a store-only probe over the same
buffer and beside the obvious torch composition of the same batch (stack, slice, flip, mul / add, where, permute().contiguous()), then times
the configs[4]-shaped step fed by a fixed batch and fed by the loader.  --loss-only times `nvnet_loss` + autograd against `nvnet_loss_hip`
(csrc/mrdis_loss3d.hip) on the net's own output shapes, the two kernels alone (achieved bytes/s from the bytes the algorithm needs) beside the
store-only probe, and prints both objectives' error against a float64 evaluation.  --fused-loss times the whole step with either objective in
alternating windows; the torch windows repeat, which gives the box's run-to-run spread.  --predict times mrdis_seg_accum (at an aligned and at
BraTS's unaligned last offset) and mrdis_seg_label_volume (csrc/mrdis_segvol.hip) beside the store-only probe over the same bytes and beside the
torch composition of the same batch, in alternating windows, then predict_volumes of one batch at stride 32 with and without the flip.  One JSON
line per measurement.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mrdis  # noqa: E402


def timeit(fn, reps):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3          # us


def layer_table(B, S, c, reps):
    dev = torch.device('cuda:0')
    geoms = [('conv1a', 4, c, S, 1)]
    for lvl, mult in enumerate((1, 2, 4, 8)):
        s = S >> lvl
        geoms.append((f'block{lvl + 1} {c * mult}->{c * mult}', c * mult, c * mult, s, 1))
        if lvl < 3:
            geoms.append((f'ds{lvl + 1}', c * mult, c * mult * 2, s, 2))
    for lvl, mult in enumerate((8, 4, 2)):
        geoms.append((f'vconv{3 - lvl} {c * mult}->{c * mult // 2}', c * mult, c * mult // 2, S >> (3 - lvl), 1))
    geoms.append(('hidden_conv', c * 8, c * 4, S >> 3, 1))
    rows = []
    for name, ci, co, s, st in geoms:
        x = torch.randn(B, s, s, s, ci, device=dev).permute(0, 4, 1, 2, 3)
        w = torch.randn(co, ci, 3, 3, 3, device=dev) * 0.1
        one = torch.ones(1, device=dev)
        w_tck, w_tkc = mrdis.hip.mix_experts_fwd(w.reshape(1, co, ci, 27, 1), one)
        bias = torch.zeros(co, device=dev)
        y = mrdis.hip.conv3d_fwd(x, w_tck, bias, 3, st, 1)
        dy = torch.randn_like(y)
        so = y.shape[2]
        flop = 2.0 * B * so ** 3 * 27 * ci * co
        t_f = timeit(lambda: mrdis.hip.conv3d_fwd(x, w_tck, bias, 3, st, 1), reps)
        t_d = timeit(lambda: mrdis.hip.conv3d_bwd_data(dy, w_tkc, tuple(x.shape), 3, st, 1), reps)
        t_w = timeit(lambda: mrdis.hip.conv3d_bwd_weight(x, dy, 3, st, 1, True), reps)
        mb = 4.0 * (x.numel() + y.numel()) / 1e6
        # roofline leg (round 6): direct-convolution FLOPs / time against the fp32 MFMA peak (157.3 TF/s; the hybrid Winograd and the six-product kernels execute
        # fewer / cheaper multiplies, so their fraction can exceed what an fp32 MFMA kernel could reach) and algorithmic bytes (x + y, fp32) / time against 8 TB/s
        frac = lambda t: (round(flop / t / 1e6 / 157.3, 3), round(mb / t * 1e3 / 8000.0, 3))
        rows.append(dict(layer=name, ci=ci, co=co, size=s, stride=st, gflop=round(flop / 1e9, 2), mb=round(mb, 1),
                         fwd_us=round(t_f, 1), dgrad_us=round(t_d, 1), wgrad_us=round(t_w, 1),
                         fwd_tf=round(flop / t_f / 1e6, 1), dgrad_tf=round(flop / t_d / 1e6, 1), wgrad_tf=round(flop / t_w / 1e6, 1),
                         fwd_gbs=round(mb / t_f * 1e3, 0),
                         fwd_frac_mfma_hbm=frac(t_f), dgrad_frac_mfma_hbm=frac(t_d), wgrad_frac_mfma_hbm=frac(t_w),
                         bound='mfma' if flop / (mb * 1e6) > 157.3e12 / 8e12 else 'hbm'))
        print(json.dumps(rows[-1]), flush=True)
        del x, y, dy
    return rows


def torch_batch(store, ds, metas):
    """the loader's batch as the obvious torch composition (what a user would write without the gather kernel)"""
    H, W, D = store.shape
    z0, Dz = ds.crop()
    xs = []
    for sid, _, ptrs, drop, tptr, flip, scale, shift in metas:
        vols = [store.vols.get(sid + '/' + c) if m != drop else None for m, c in enumerate(ds.contrast_list)]
        raw = torch.stack([v[:, :, z0:z0 + Dz] if v is not None else torch.zeros(H, W, Dz, device=store.device) for v in vols])
        if flip:
            raw = raw.flip(1)
        x = raw * scale + shift
        xs.append(torch.where(raw == raw.min(), torch.full_like(x, -10.0), x))
    return torch.stack(xs).permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3)


def loader_bench(a):
    import numpy as np
    dev = torch.device('cuda:0')
    H, W, D = a.vol
    B, M, nsubj = a.batch, 4, 8
    contrasts = ['T1', 'T1c', 'T2', 'T2_FLAIR']
    g = torch.Generator().manual_seed(2)
    store = mrdis.VolumeStore3D(dev)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing='ij')
    inside = (((yy - H / 2) / (0.4 * H)) ** 2 + ((xx - W / 2) / (0.42 * W)) ** 2 <= 1)[:, :, None]
    for s in range(nsubj):
        for ci, c in enumerate(contrasts):
            if (s + ci) % 5 == 0:
                continue                                     # a missing contrast now and then
            store.add(f's{s:02d}/{c}', torch.where(inside, torch.randn(H, W, D, generator=g), torch.tensor(-10.0)).numpy())
        store.add(f's{s:02d}/seg', (torch.randint(0, 5, (H, W, D), generator=g) * inside).float().numpy())
    ds = mrdis.VolumeDataset3D('BraTS', store, [f's{s:02d}' for s in range(nsubj)], contrasts, aug=True, dropoff=True)
    loader = mrdis.VolumeLoader3D(ds, B, shuffle=True, region_channels=3)
    z0, Dz = ds.crop()
    np.random.seed(1); torch.manual_seed(1)
    _, _, metas = next(iter(loader.batch_plan()))
    tab = torch.from_numpy(loader.table(metas)[0]).to(dev)
    x, _ = mrdis.hip.volume_gather(tab, M, H, W, D, z0, Dz)
    want = torch_batch(store, ds, [(m[0], m[1], m[2], m[3], m[4], m[5], float(np.float32(m[6])), float(np.float32(m[7]))) for m in metas])
    assert torch.equal(x, want), 'gather and torch composition disagree'
    present = sum(1 for m in metas for k, p in enumerate(m[2]) if p and k != m[3])
    moved = 4.0 * H * W * Dz * (present + B * M)              # bytes the algorithm needs: every present crop read once, the batch written once
    out_buf = torch.empty(B * H * W * Dz * M, device=dev)
    t_fill = timeit(lambda: mrdis.hip.stream_fill(out_buf), a.reps)
    rows = []
    for gen, name in ((0, 'gather (LDS tile kernel)'), (1, 'gather (element kernel)')):
        with mrdis.hip.option('debug_volgen', gen):
            t = timeit(lambda: mrdis.hip.volume_gather(tab, M, H, W, D, z0, Dz), a.reps)
        rows.append({'metric': name, 'us': round(t, 1), 'moved_mb': round(moved / 1e6, 1), 'tb_per_s': round(moved / t / 1e6, 2)})
    t_tgt = timeit(lambda: mrdis.hip.volume_gather(tab, M, H, W, D, z0, Dz, targets=True, K=3, relabel=True), a.reps)
    rows.append({'metric': 'target gather, 3 region channels', 'us': round(t_tgt, 1)})
    rows.append({'metric': 'store-only probe over the batch buffer', 'us': round(t_fill, 1), 'written_mb': round(4.0 * out_buf.numel() / 1e6, 1),
                 'tb_per_s': round(4.0 * out_buf.numel() / t_fill / 1e6, 2)})
    t_torch = timeit(lambda: torch_batch(store, ds, metas), a.reps)
    rows.append({'metric': 'torch composition of the same batch', 'us': round(t_torch, 1), 'over_gather': round(t_torch / rows[0]['us'], 2)})
    for r in rows:
        r['config'] = f'B={B} M={M} {H}x{W}x{D} (Dz={Dz}) fp32'
        print(json.dumps(r), flush=True)
    if a.steps < 1:
        return
    # the configs[4]-shaped step (NVNet3D, init_channels 16) on this batch shape: fed by one fixed batch, then with the loader in the loop
    torch.manual_seed(10)
    model = mrdis.NVNet3D((H, W, Dz), M, 3, a.channels, p=0.2).to(dev).train()
    opt = mrdis.ArenaAdam(model.parameters(), lr=1e-4, weight_decay=1e-5)

    def step(x, t):
        loss, _ = mrdis.nvnet_loss(*model(x), x, t)
        loss.backward()
        opt.step(fused_clip=True)
        opt.zero_grad()
        return loss

    def batches():
        while True:
            yield from loader

    it = batches()
    b0 = next(it)
    for _ in range(a.warmup):
        step(b0['inputs'], b0['targets'])
    res = {}
    for name in ('fixed batch', 'loader in the loop', 'fixed batch', 'loader in the loop'):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            b = b0 if name == 'fixed batch' else next(it)
            loss = step(b['inputs'], b['targets'])
        torch.cuda.synchronize()
        res.setdefault(name, []).append((time.perf_counter() - t0) / a.steps * 1e3)
    print(json.dumps({'metric': 'NVNet3D train step, ms (two alternating windows each)', 'fixed_batch': [round(v, 2) for v in res['fixed batch']],
                      'loader_in_loop': [round(v, 2) for v in res['loader in the loop']], 'steps_per_window': a.steps,
                      'config': f'B={B} M={M} {H}x{W}x{Dz} fp32, init_channels {a.channels}', 'loss': float(loss.detach())}), flush=True)


def loss_f64(uout, vout, mu, logvar, x, target):
    """`nvnet_loss` evaluated in float64 with autograd: (loss, d loss / d uout, d loss / d vout)"""
    u = uout.detach().double().requires_grad_(True)
    v = vout.detach().double().requires_grad_(True)
    loss, _ = mrdis.nvnet_loss(u, v, mu.double(), logvar.double(), x.double(), target.double())
    loss.backward()
    return loss.detach(), u.grad, v.grad


def loss_inputs(B, S, dev, seed=1):
    g = torch.Generator().manual_seed(seed)
    mk = lambda c: torch.randn(B, S, S, S, c, generator=g).to(dev).permute(0, 4, 1, 2, 3)
    uout, vout, x = mk(3), mk(4), mk(4)
    t = (torch.rand(B, S, S, S, 3, generator=g) > 0.7).float().to(dev).permute(0, 4, 1, 2, 3)
    mu, logvar = torch.randn(B, 16, generator=g).to(dev), (0.1 * torch.randn(B, 16, generator=g)).to(dev)
    return uout, vout, mu, logvar, x, t


def loss_bench(a):
    dev = torch.device('cuda:0')
    B, S = a.batch, a.size
    uout, vout, mu, logvar, x, t = loss_inputs(B, S, dev)
    cfgs = f'{B}x3x{S}^3 + {B}x4x{S}^3 fp32 channels-last-3d'

    def run(fn):
        u = uout.detach().requires_grad_(True); v = vout.detach().requires_grad_(True)
        loss, _ = fn(u, v, mu, logvar, x, t)
        loss.backward()
        return loss.detach(), u.grad, v.grad

    # parity of both objectives against float64 (the yardstick of tests/test_gpu_loss3d.py)
    l64, du64, dv64 = loss_f64(uout, vout, mu, logvar, x, t)
    err = {}
    for name, fn in (('torch', mrdis.nvnet_loss), ('fused', mrdis.nvnet_loss_hip)):
        l, du, dv = run(fn)
        err[name] = dict(loss_rel=float(((l.double() - l64) / l64).abs()), du_max_abs=float((du.double() - du64).abs().max()),
                         dv_max_abs=float((dv.double() - dv64).abs().max()))
    print(json.dumps({'metric': 'objective error against float64', 'config': cfgs, 'loss_f64': float(l64), 'du_max_f64': float(du64.abs().max()),
                      'dv_max_f64': float(dv64.abs().max()), **{f'{k}_{n}': v for n, e in err.items() for k, v in e.items()}}), flush=True)
    del l64, du64, dv64
    # forward + backward per call, alternating (torch, fused) x 3: the repeats give the spread
    rows = {'torch': [], 'fused': []}
    for _ in range(3):
        for name, fn in (('torch', mrdis.nvnet_loss), ('fused', mrdis.nvnet_loss_hip)):
            rows[name].append(round(timeit(lambda: run(fn), a.reps), 1))
    print(json.dumps({'metric': 'objective forward + backward, us per call (three alternating windows)', 'config': cfgs, 'torch_nvnet_loss': rows['torch'],
                      'fused_nvnet_loss_hip': rows['fused'], 'reps_per_window': a.reps,
                      'torch_over_fused': round(min(rows['torch']) / min(rows['fused']), 2)}), flush=True)
    # the two kernels alone, and the store-only probe over a buffer as large as what the backward writes
    n1, n2 = uout.numel(), vout.numel()
    sums, _ = mrdis.hip.nvnet_loss_fwd(uout, t, vout, x)
    gone = torch.ones(1, device=dev)
    t_f = timeit(lambda: mrdis.hip.nvnet_loss_fwd(uout, t, vout, x), a.reps)
    t_b = timeit(lambda: mrdis.hip.nvnet_loss_bwd(gone, sums, uout, t, vout, x), a.reps)
    buf = torch.empty(n1 + n2, device=dev)
    t_s = timeit(lambda: mrdis.hip.stream_fill(buf), a.reps)
    t_e = timeit(lambda: torch.empty_like(uout), a.reps)
    rd, wr = 4.0 * 2 * (n1 + n2), 4.0 * (n1 + n2)
    print(json.dumps({'metric': 'mrdis_nvnet_loss_fwd (kernel + finish)', 'us': round(t_f, 1), 'read_mb': round(rd / 1e6, 1), 'tb_per_s': round(rd / t_f / 1e6, 2)}), flush=True)
    print(json.dumps({'metric': 'mrdis_nvnet_loss_bwd (incl. two torch.empty_like)', 'us': round(t_b, 1), 'read_mb': round(rd / 1e6, 1), 'written_mb': round(wr / 1e6, 1),
                      'tb_per_s': round((rd + wr) / t_b / 1e6, 2), 'empty_like_us': round(t_e, 1)}), flush=True)
    print(json.dumps({'metric': 'store-only probe over du + dv bytes', 'us': round(t_s, 1), 'written_mb': round(wr / 1e6, 1), 'tb_per_s': round(wr / t_s / 1e6, 2)}), flush=True)
    tc = (torch.rand(B, S, S, S, 3, device=dev) > 0.5).float().permute(0, 4, 1, 2, 3)
    t_c = timeit(lambda: mrdis.hip.seg_counts(uout, tc, logits=True), a.reps)
    print(json.dumps({'metric': 'mrdis_seg_counts (logits, incl. zeroing the counts)', 'us': round(t_c, 1), 'read_mb': round(8.0 * n1 / 1e6, 1),
                      'tb_per_s': round(8.0 * n1 / t_c / 1e6, 2)}), flush=True)


def step_bench(a):
    """the NVNet3D step with the torch objective (what the parent ran) and with the fused one: alternating windows torch, fused, torch, fused, torch"""
    dev = torch.device('cuda:0')
    S, B = a.size, a.batch
    torch.manual_seed(10)
    model = mrdis.NVNet3D((S, S, S), 4, 3, a.channels, p=0.2).to(dev).train()
    opt = mrdis.ArenaAdam(model.parameters(), lr=1e-4, weight_decay=1e-5)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, S, S, S, 4, generator=g).to(dev).permute(0, 4, 1, 2, 3)
    t = (torch.rand(B, S, S, S, 3, generator=g) > 0.7).float().to(dev).permute(0, 4, 1, 2, 3)

    def step(fn):
        loss, _ = fn(*model(x), x, t)
        loss.backward()
        opt.step(fused_clip=True)
        opt.zero_grad()
        return loss

    for _ in range(a.warmup):
        step(mrdis.nvnet_loss); step(mrdis.nvnet_loss_hip)
    res = {'torch': [], 'fused': []}
    for name in ('torch', 'fused', 'torch', 'fused', 'torch'):
        fn = mrdis.nvnet_loss if name == 'torch' else mrdis.nvnet_loss_hip
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            loss = step(fn)
        torch.cuda.synchronize()
        res[name].append(round((time.perf_counter() - t0) / a.steps * 1e3, 2))
    print(json.dumps({'metric': 'NVNet3D train step, ms (alternating windows)', 'torch_objective': res['torch'], 'fused_objective': res['fused'],
                      'torch_spread_ms': round(max(res['torch']) - min(res['torch']), 2), 'steps_per_window': a.steps,
                      'config': f'{B}x4x{S}^3 fp32, init_channels {a.channels}, dropout 0.2', 'loss': float(loss.detach())}), flush=True)


def predict_bench(a):
    """the kernels of csrc/mrdis_segvol.hip at B x 3 x H x W, Dz = 64, D from --vol: achieved bytes/s from the bytes the algorithm needs"""
    dev = torch.device('cuda:0')
    H, W, D = a.vol
    B, C, Dz = a.batch, 3, 64
    hip = mrdis.hip
    g = torch.Generator().manual_seed(4)
    logits = (3 * torch.randn(B, H, W, Dz, C, generator=g)).to(dev).permute(0, 4, 1, 2, 3)
    acc = torch.zeros(B, H, W, D, C, device=dev)
    win = 4.0 * logits.numel()
    cfgs = f'{B} x {C} x {H} x {W}, Dz {Dz}, D {D}'
    z_al, z_un = 32, D - Dz

    def torch_accum(z0, flip=False):
        p = torch.sigmoid(logits.permute(0, 2, 3, 4, 1))
        acc[:, :, :, z0:z0 + Dz] += p.flip(1) if flip else p

    buf = torch.empty(int(3 * win / 4) // 4 * 4, device=dev)
    rows = {'kernel_z%d' % z_al: [], 'kernel_z%d' % z_un: [], 'kernel_z%d_flip' % z_un: [], 'torch_z%d' % z_un: [], 'store_only': []}
    for _ in range(3):                                          # alternating windows: the repeats give the spread
        rows['kernel_z%d' % z_al].append(round(timeit(lambda: hip.seg_accum(logits, acc, z_al), a.reps), 1))
        rows['kernel_z%d' % z_un].append(round(timeit(lambda: hip.seg_accum(logits, acc, z_un), a.reps), 1))
        rows['kernel_z%d_flip' % z_un].append(round(timeit(lambda: hip.seg_accum(logits, acc, z_un, flip_h=True), a.reps), 1))
        rows['torch_z%d' % z_un].append(round(timeit(lambda: torch_accum(z_un), a.reps), 1))
        rows['store_only'].append(round(timeit(lambda: hip.stream_fill(buf), a.reps), 1))
    best = {k: min(v) for k, v in rows.items()}
    print(json.dumps({'metric': 'mrdis_seg_accum, us per call (three alternating windows)', 'config': cfgs, **rows,
                      'moved_mb': round(3 * win / 1e6, 1), 'note': 'moved = logits read + acc window read + acc window write',
                      'tb_per_s': {k: round(3 * win / t / 1e6, 2) for k, t in best.items() if k.startswith('kernel')},
                      'store_only_tb_per_s': round(4.0 * buf.numel() / best['store_only'] / 1e6, 2),
                      'torch_over_kernel': round(best['torch_z%d' % z_un] / best['kernel_z%d' % z_un], 2)}), flush=True)
    # labels + counts
    acc.zero_()
    offs = mrdis.window_offsets(D, Dz, 32)
    for z0 in offs:
        hip.seg_accum(logits, acc, z0)
    cover = torch.from_numpy(mrdis.model3d.window_cover(D, Dz, offs)).to(dev)
    vols = [torch.randint(0, 5, (H, W, D), generator=g).float().to(dev) for _ in range(B)]
    ptrs = torch.tensor([v.data_ptr() for v in vols], dtype=torch.int64).to(dev)
    tvol = torch.stack(vols)

    def torch_labels():
        pbar = acc / cover.float().view(1, 1, 1, D, 1)
        pred = pbar > 0.5
        t = torch.where(tvol == 4, torch.full_like(tvol, 3.0), tvol)
        lab = torch.stack([t == c + 1 for c in range(C)], dim=-1)
        mx, arg = pbar.max(dim=-1)
        labels = torch.where(mx > 0.5, arg + 1, torch.zeros_like(arg))
        labels = torch.where(labels == 3, torch.full_like(labels, 4), labels).to(torch.uint8)
        counts = torch.stack([(pred & lab).flatten(1, 3).sum(1), pred.flatten(1, 3).sum(1), lab.flatten(1, 3).sum(1)], dim=-1)
        return labels, counts

    lk, ck = hip.seg_label_volume(acc, cover, ptrs, relabel=True)
    lt, ct = torch_labels()
    moved = 4.0 * acc.numel() + 4.0 * tvol.numel() + 1.0 * tvol.numel()
    buf2 = torch.empty(int(moved / 4) // 4 * 4, device=dev)
    rows = {'kernel': [], 'torch': [], 'store_only': []}
    for _ in range(3):
        rows['kernel'].append(round(timeit(lambda: hip.seg_label_volume(acc, cover, ptrs, relabel=True), a.reps), 1))
        rows['torch'].append(round(timeit(torch_labels, a.reps), 1))
        rows['store_only'].append(round(timeit(lambda: hip.stream_fill(buf2), a.reps), 1))
    best = {k: min(v) for k, v in rows.items()}
    print(json.dumps({'metric': 'mrdis_seg_label_volume (incl. zeroing the counts), us per call (three alternating windows)', 'config': cfgs, **rows,
                      'moved_mb': round(moved / 1e6, 1), 'note': 'moved = acc read + ground truth read + labels written',
                      'tb_per_s': round(moved / best['kernel'] / 1e6, 2), 'store_only_tb_per_s': round(4.0 * buf2.numel() / best['store_only'] / 1e6, 2),
                      'torch_over_kernel': round(best['torch'] / best['kernel'], 2),
                      'labels_differ_from_torch': int((lk != lt).sum()), 'counts_equal_torch': bool(torch.equal(ck.long(), ct.long()))}), flush=True)
    del buf, buf2, acc, logits, tvol, vols
    # one batch end to end: gather, the net's unet and the accumulation per window (and flip), then the label volume
    contrasts = ['T1', 'T1c', 'T2', 'T2_FLAIR']
    store = mrdis.VolumeStore3D(dev)
    for s_ in range(B):
        for c in contrasts:
            store.add(f's{s_:02d}/{c}', torch.randn(H, W, D, generator=g).numpy())
        store.add(f's{s_:02d}/seg', torch.randint(0, 5, (H, W, D), generator=g).float().numpy())
    ds = mrdis.VolumeDataset3D('BraTS', store, [f's{s_:02d}' for s_ in range(B)], contrasts)
    loader = mrdis.VolumeLoader3D(ds, B, region_channels=3)
    torch.manual_seed(10)
    model = mrdis.NVNet3D((H, W, ds.crop()[1]), 4, 3, a.channels, p=0.2).to(dev)

    def whole(flip):
        for r in mrdis.predict_volumes(model, loader, stride=32, flip=flip):
            last = r['labels']
        torch.cuda.synchronize()
        return last

    whole(False); whole(True)
    rows = {'no_flip_ms': [], 'flip_ms': []}
    for _ in range(3):
        for key, f in (('no_flip_ms', False), ('flip_ms', True)):
            t0 = time.perf_counter()
            for _ in range(a.steps):
                whole(f)
            rows[key].append(round((time.perf_counter() - t0) / a.steps * 1e3, 1))
    print(json.dumps({'metric': 'predict_volumes, ms per batch (three alternating windows)', 'config': cfgs + f', stride 32, init_channels {a.channels}',
                      'windows': len(offs), **rows}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=128)
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--channels', type=int, default=16)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--layers', action='store_true')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--loader', action='store_true')
    ap.add_argument('--loss-only', action='store_true', help='time the objective (forward + backward): torch composition vs fused HIP kernels')
    ap.add_argument('--fused-loss', action='store_true', help='time the step with the torch objective and with the fused one')
    ap.add_argument('--predict', action='store_true', help='time whole-volume sliding-window prediction (csrc/mrdis_segvol.hip)')
    ap.add_argument('--vol', type=int, nargs=3, default=[160, 192, 155], help='--loader: H W D of the stored volumes')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X (no CPU fallback)'
    dev = torch.device('cuda:0')
    mrdis.hip.load()
    if a.layers:
        layer_table(a.batch, a.size, a.channels, a.reps)
        return
    if a.loader:
        loader_bench(a)
        return
    if a.loss_only:
        loss_bench(a)
        return
    if a.fused_loss:
        step_bench(a)
        return
    if a.predict:
        predict_bench(a)
        return
    S, B = a.size, a.batch
    torch.manual_seed(10)
    model = mrdis.NVNet3D((S, S, S), 4, 3, a.channels, p=0.2).to(dev).train()
    opt = mrdis.ArenaAdam(model.parameters(), lr=1e-4, weight_decay=1e-5)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, S, S, S, 4, generator=g).to(dev).permute(0, 4, 1, 2, 3)
    t = (torch.rand(B, S, S, S, 3, generator=g) > 0.7).float().to(dev).permute(0, 4, 1, 2, 3)

    def step():
        out = model(x)
        loss, _ = mrdis.nvnet_loss(*out, x, t)
        loss.backward()
        opt.step(fused_clip=True)
        opt.zero_grad()
        return loss

    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        loss = step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.steps
    print(json.dumps({'metric': 'NVNet3D train step', 'ms_per_step': round(dt * 1e3, 2), 'volumes_per_s': round(B / dt, 2),
                      'config': {'workload': f'{B}x4x{S}^3 fp32, init_channels {a.channels}, dropout 0.2'},
                      'loss': float(loss), 'peak_mem_gib': round(torch.cuda.max_memory_allocated() / 2 ** 30, 1)}))


if __name__ == '__main__':
    main()
