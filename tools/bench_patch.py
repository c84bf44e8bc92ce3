"""Timing of patch sampling for the 3-D nets (csrc/mrdis_patch.hip, patch3d.py, data3d.py's patch mode) on one MI355X:

    python tools/bench_patch.py [--batch 4] [--vol 160 192 155] [--patch 128 128 128] [--out profiles/patch_bench.txt]

Builds a synthetic BraTS-shaped store and times, in alternating windows inside ONE run (the repeats give the box's spread):
the one-off prefix-table build per subject; mrdis_patch_origins; mrdis_patch_gather for the inputs and for the targets, each beside a
store-only pass over the same bytes (mrdis_stream_fill) and beside the torch composition of the same batch (index, flip, mul / add, where,
permute); then the NVNet3D step on a fixed batch against the same step with the patch loader in the loop.  One JSON line per result; with
--out the lines are also written to that file.  No threshold: the numbers are recorded as they come out.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mrdis  # noqa: E402

CONTRASTS = ['T1', 'T1c', 'T2', 'T2_FLAIR']
CLASSES = (1, 2, 4)


def timeit(fn, reps):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3          # us


def build_store(dev, H, W, D, nsubj):
    """z-scored values inside an ellipse, -10 outside, a missing contrast now and then; a tumour blob of the three classes per subject"""
    g = torch.Generator().manual_seed(2)
    store = mrdis.VolumeStore3D(dev)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing='ij')
    inside = (((yy - H / 2) / (0.4 * H)) ** 2 + ((xx - W / 2) / (0.42 * W)) ** 2 <= 1)[:, :, None]
    for s in range(nsubj):
        for ci, c in enumerate(CONTRASTS):
            if (s + ci) % 5 == 0:
                continue
            store.add(f's{s:02d}/{c}', torch.where(inside, torch.randn(H, W, D, generator=g), torch.tensor(-10.0)).numpy())
        seg = torch.zeros(H, W, D)
        h, w, d = H // 3 + 5 * s, W // 3 + 4 * s, D // 3 + 3 * s
        blob = torch.randint(0, 5, (H // 5, W // 5, D // 5), generator=g).float()
        blob[blob == 3] = 0
        seg[h:h + H // 5, w:w + W // 5, d:d + D // 5] = blob
        store.add(f's{s:02d}/seg', seg.numpy())
    return store


def torch_batch(store, ds, metas, origins, patch, targets=False, mins=None):
    """the patch batch as the obvious torch composition over the same draws: index, flip, mul / add, where, permute.  `origins`: host integers;
    `mins`: {key: whole-volume minimum} as host floats, made once (the loader keeps them on the device)."""
    PH, PW, PD = patch
    xs = []
    for (sid, _, ptrs, drop, tptr, _, scale, shift, (fg, u, flips, centre)), (h0, w0, d0, _) in zip(metas, origins):
        dims = [i + 1 for i, f in enumerate(flips) if f]
        if targets:
            seg = store.vols.get(sid + '/seg')
            t = seg[h0:h0 + PH, w0:w0 + PW, d0:d0 + PD] if seg is not None else torch.zeros(patch, device=store.device)
            t = torch.where(t == 4, torch.full_like(t, 3.0), t)
            t = torch.stack([(t == c + 1).float() for c in range(3)])
            xs.append(t.flip(dims) if dims else t)
            continue
        vols = [store.vols.get(sid + '/' + c) if m != drop else None for m, c in enumerate(ds.contrast_list)]
        raw = torch.stack([v[h0:h0 + PH, w0:w0 + PW, d0:d0 + PD] if v is not None else torch.zeros(patch, device=store.device) for v in vols])
        if dims:
            raw = raw.flip(dims)
        m0 = min([mins[sid + '/' + c] for m, c in enumerate(ds.contrast_list) if vols[m] is not None] + ([0.0] if any(v is None for v in vols) else []))
        x = raw * scale + shift
        xs.append(torch.where(raw == m0, torch.full_like(x, -10.0), x))
    return torch.stack(xs).permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--vol', type=int, nargs=3, default=[160, 192, 155])
    ap.add_argument('--patch', type=int, nargs=3, default=[128, 128, 128])
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--windows', type=int, default=3)
    ap.add_argument('--steps', type=int, default=10, help='NVNet3D steps per window; 0: skip the step')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--channels', type=int, default=16)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    H, W, D = a.vol
    patch = tuple(a.patch)
    PH, PW, PD = patch
    B, M, nsubj = a.batch, 4, 8
    lines = []

    def emit(row):
        row['config'] = f'B={B} M={M} store {H}x{W}x{D} patch {PH}x{PW}x{PD} fp32'
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    store = build_store(dev, H, W, D, nsubj)
    ds = mrdis.VolumeDataset3D('BraTS', store, [f's{s:02d}' for s in range(nsubj)], CONTRASTS, aug=True, dropoff=True)
    loader = mrdis.VolumeLoader3D(ds, B, shuffle=True, region_channels=3, patch_size=patch, patch_fg=0.33, patch_flips='hwd')
    p = mrdis.patch3d

    # the one-off table build per subject: the counting kernel alone, and with the running sum
    seg = store.vols['s00/seg']
    rows = {'fg_block_counts': [], 'fg_prefix (counts + cumsum)': []}
    for _ in range(a.windows):
        rows['fg_block_counts'].append(round(timeit(lambda: p.fg_block_counts(seg, CLASSES), a.reps), 1))
        rows['fg_prefix (counts + cumsum)'].append(round(timeit(lambda: p.fg_prefix(seg, CLASSES), a.reps), 1))
    nblk = (H * W * D + p.BLOCK - 1) // p.BLOCK
    emit({'metric': 'prefix-table build per subject, us (alternating windows)', **rows, 'read_mb': round(4.0 * H * W * D / 1e6, 1),
          'table_kb': round(4.0 * (nblk + 1) * len(CLASSES) / 1e3, 1)})

    np.random.seed(1); torch.manual_seed(1)
    _, _, metas = next(iter(loader.batch_plan()))
    tab = torch.from_numpy(loader.patch_table(metas)[0]).to(dev)
    origins = p.patch_origins(tab, M, store.shape, patch, CLASSES)
    o_host = origins.cpu().tolist()
    x, _ = p.patch_gather(tab, origins, M, store.shape, patch)
    t = p.patch_gather(tab, origins, M, store.shape, patch, targets=True, K=3, relabel=True)
    mins = {k: float(v.min()) for k, v in store.vols.items()}
    f32 = lambda m: m[:6] + (float(np.float32(m[6])), float(np.float32(m[7]))) + m[8:]
    assert torch.equal(x, torch_batch(store, ds, [f32(m) for m in metas], o_host, patch, mins=mins)), 'gather and torch composition disagree (inputs)'
    assert torch.equal(t, torch_batch(store, ds, metas, o_host, patch, targets=True)), 'gather and torch composition disagree (targets)'

    present = sum(1 for m in metas for k, ptr in enumerate(m[2]) if ptr and k != m[3])
    N = PH * PW * PD
    in_buf, tg_buf = torch.empty(B * N * M, device=dev), torch.empty(B * N * 3, device=dev)
    rows = {k: [] for k in ('patch_origins', 'inputs: gather (LDS tile)', 'inputs: gather (element form)', 'inputs: store-only', 'inputs: torch composition',
                            'targets: gather (LDS tile)', 'targets: store-only', 'targets: torch composition')}
    for _ in range(a.windows):
        rows['patch_origins'].append(timeit(lambda: p.patch_origins(tab, M, store.shape, patch, CLASSES), a.reps))
        rows['inputs: gather (LDS tile)'].append(timeit(lambda: p.patch_gather(tab, origins, M, store.shape, patch), a.reps))
        with mrdis.hip.option('debug_volgen', 1):
            rows['inputs: gather (element form)'].append(timeit(lambda: p.patch_gather(tab, origins, M, store.shape, patch), a.reps))
        rows['inputs: store-only'].append(timeit(lambda: mrdis.hip.stream_fill(in_buf), a.reps))
        rows['inputs: torch composition'].append(timeit(lambda: torch_batch(store, ds, metas, o_host, patch, mins=mins), max(a.reps // 5, 1)))
        rows['targets: gather (LDS tile)'].append(timeit(lambda: p.patch_gather(tab, origins, M, store.shape, patch, targets=True, K=3, relabel=True), a.reps))
        rows['targets: store-only'].append(timeit(lambda: mrdis.hip.stream_fill(tg_buf), a.reps))
        rows['targets: torch composition'].append(timeit(lambda: torch_batch(store, ds, metas, o_host, patch, targets=True), max(a.reps // 5, 1)))
    moved_in, moved_tg = 4.0 * N * (present + B * M), 4.0 * N * (B + B * 3)
    best = {k: min(v) for k, v in rows.items()}
    emit({'metric': 'patch batch kernels, us per call (alternating windows)', **{k: [round(v, 1) for v in vs] for k, vs in rows.items()},
          'inputs_moved_mb': round(moved_in / 1e6, 1), 'inputs_written_mb': round(4.0 * in_buf.numel() / 1e6, 1),
          'inputs_gather_tb_per_s': round(moved_in / best['inputs: gather (LDS tile)'] / 1e6, 2),
          'inputs_store_only_tb_per_s': round(4.0 * in_buf.numel() / best['inputs: store-only'] / 1e6, 2),
          'targets_moved_mb': round(moved_tg / 1e6, 1), 'targets_gather_tb_per_s': round(moved_tg / best['targets: gather (LDS tile)'] / 1e6, 2),
          'targets_store_only_tb_per_s': round(4.0 * tg_buf.numel() / best['targets: store-only'] / 1e6, 2),
          'note': 'moved = every present patch read once + the batch written once; best window for the rates'})
    del in_buf, tg_buf
    if a.steps < 1:
        return finish(a, lines)

    torch.manual_seed(10)
    model = mrdis.NVNet3D(patch, M, 3, a.channels, p=0.2).to(dev).train()
    opt = mrdis.ArenaAdam(model.parameters(), lr=1e-4, weight_decay=1e-5)

    def step(x, t):
        loss, _ = mrdis.nvnet_loss_hip(*model(x), x, t)
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
    for name in ('fixed batch', 'patch loader in the loop') * 2:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            b = b0 if name == 'fixed batch' else next(it)
            loss = step(b['inputs'], b['targets'])
        torch.cuda.synchronize()
        res.setdefault(name, []).append(round((time.perf_counter() - t0) / a.steps * 1e3, 2))
    emit({'metric': 'NVNet3D train step, ms (two alternating windows each)', 'fixed_batch': res['fixed batch'], 'patch_loader_in_loop': res['patch loader in the loop'],
          'steps_per_window': a.steps, 'init_channels': a.channels, 'loss': float(loss.detach())})
    finish(a, lines)


def finish(a, lines):
    if a.out:
        with open(a.out, 'w') as f:
            f.write('# python tools/bench_patch.py ' + ' '.join(sys.argv[1:]) + '\n' + '\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
