"""Timing of the rotated and zoomed training patches (csrc/mrdis_warp.hip, patch3d.patch_warp, data3d.py's `patch_warp` keys) on one MI355X:

    python tools/bench_warp.py [--batch 4] [--vol 160 192 155] [--patch 128 128 128] [--out profiles/warp_bench.txt]

Builds the synthetic BraTS-shaped store of tools/bench_patch.py and times, in alternating windows inside ONE run (the repeats give the box's
spread): mrdis_patch_warp for the inputs and for the targets with every row warped (30 degrees about each axis, zoom 0.7 and zoom 1.4) and
with no row warped, in its LDS-tile and its element form; mrdis_patch_gather on the same table; a store-only pass over the output bytes
(mrdis_stream_fill); the torch composition of a warped batch (affine_grid + grid_sample, bilinear and nearest per item, plus the background
rule); then the NVNet3D step on a fixed batch against the same step with the warping loader in the loop.  One JSON line per result; with
--out the lines are also written to that file.  No threshold: the numbers are recorded as they come out.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mrdis  # noqa: E402
from bench_patch import CLASSES, CONTRASTS, build_store, timeit  # noqa: E402


def torch_batch(store, ds, metas, origins, patch, mins):
    """a warped batch as the obvious torch composition over the same draws: per item one affine_grid, grid_sample bilinear over the present
    contrasts, grid_sample nearest over the same stack for the background rule (-10 where the nearest raw voxel is the minimum), grid_sample
    nearest over the label volume, the region channels.  Float coordinates: close to the kernel's batch, not equal to it."""
    PH, PW, PD = patch
    H, W, D = store.shape
    dims, P = (H, W, D), (PH, PW, PD)
    xs, ts = [], []
    for (sid, _, ptrs, drop, tptr, _, scale, shift, (fg, u, flips, centre, warp, angles, zoom)), (h0, w0, d0, _) in zip(metas, origins):
        A = mrdis.patch3d.warp_matrix(angles, zoom).astype(np.float64) / 65536.0 if warp else np.eye(3)
        o = (h0, w0, d0)
        theta = np.zeros((3, 4))
        for r in range(3):                                          # rows and columns in grid_sample's (x, y, z) = (d, w, h) order
            for c in range(3):
                theta[2 - r, 2 - c] = A[r, c] * (P[c] - 1) / max(dims[r] - 1, 1) * (-1 if flips[c] else 1)
            theta[2 - r, 3] = 2 * (o[r] + (P[r] - 1) / 2) / max(dims[r] - 1, 1) - 1
        grid = F.affine_grid(torch.tensor(theta, dtype=torch.float32, device=store.device)[None], (1, 1, PH, PW, PD), align_corners=True)
        vols = [store.vols.get(sid + '/' + c) if m != drop else None for m, c in enumerate(ds.contrast_list)]
        stack = torch.stack([v if v is not None else torch.zeros(dims, device=store.device) for v in vols])[None]
        lin = F.grid_sample(stack, grid, mode='bilinear', padding_mode='border', align_corners=True)[0]
        near = F.grid_sample(stack, grid, mode='nearest', padding_mode='border', align_corners=True)[0]
        m0 = min([mins[sid + '/' + c] for m, c in enumerate(ds.contrast_list) if vols[m] is not None] + ([0.0] if any(v is None for v in vols) else []))
        x = lin * scale + shift
        xs.append(torch.where(near == m0, torch.full_like(x, -10.0), x))
        seg = store.vols.get(sid + '/seg')
        t = F.grid_sample(seg[None, None], grid, mode='nearest', padding_mode='border', align_corners=True)[0, 0] if seg is not None else torch.zeros(patch, device=store.device)
        t = torch.where(t == 4, torch.full_like(t, 3.0), t)
        ts.append(torch.stack([(t == c + 1).float() for c in range(3)]))
    cl = lambda v: torch.stack(v).permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3)
    return cl(xs), cl(ts)


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
    loader = mrdis.VolumeLoader3D(ds, B, shuffle=True, region_channels=3, patch_size=patch, patch_fg=0.33, patch_flips='hwd', patch_warp=1.0)
    p = mrdis.patch3d

    np.random.seed(1); torch.manual_seed(1)
    _, _, metas = next(iter(loader.batch_plan()))
    with_warp = lambda warp, zoom: [m[:8] + (m[8][:4] + (warp, (30.0, 30.0, 30.0), zoom),) for m in metas]
    table = lambda ms: torch.from_numpy(loader.patch_table(ms)[0]).to(dev)
    tabs = {'30 deg, zoom 0.7': table(with_warp(True, 0.7)), '30 deg, zoom 1.4': table(with_warp(True, 1.4)), 'no row warped': table(with_warp(False, 1.0))}
    origins = p.patch_origins(tabs['no row warped'], M, store.shape, patch, CLASSES)
    o_host = origins.cpu().tolist()
    mins = {k: float(v.min()) for k, v in store.vols.items()}
    shape = store.shape
    # sanity, not a test: rows without the flag are patch_gather's bits; the torch composition lands near the kernel's batch
    x0, _ = p.patch_warp(tabs['no row warped'], origins, M, shape, patch)
    assert torch.equal(x0, p.patch_gather(tabs['no row warped'], origins, M, shape, patch)[0])
    xk, _ = p.patch_warp(tabs['30 deg, zoom 1.4'], origins, M, shape, patch)
    tk = p.patch_warp(tabs['30 deg, zoom 1.4'], origins, M, shape, patch, targets=True, K=3, relabel=True)
    xt, tt = torch_batch(store, ds, with_warp(True, 1.4), o_host, patch, mins)
    emit({'metric': 'torch composition against the kernel, 30 deg zoom 1.4 (float against integer coordinates)',
          'inputs_share_beyond_1e-3': round(float(((xk - xt).abs() > 1e-3).float().mean()), 5), 'targets_share_different': round(float((tk != tt).float().mean()), 5)})
    del x0, xk, tk, xt, tt

    present = sum(1 for m in metas for k, ptr in enumerate(m[2]) if ptr and k != m[3])
    N = PH * PW * PD
    in_buf, tg_buf = torch.empty(B * N * M, device=dev), torch.empty(B * N * 3, device=dev)
    rows = {}
    add = lambda k, v: rows.setdefault(k, []).append(v)
    tg = dict(targets=True, K=3, relabel=True)
    for _ in range(a.windows):
        for name, tab in tabs.items():
            add(f'inputs: warp, {name} (LDS tile)', timeit(lambda: p.patch_warp(tab, origins, M, shape, patch), a.reps))
            add(f'targets: warp, {name} (LDS tile)', timeit(lambda: p.patch_warp(tab, origins, M, shape, patch, **tg), a.reps))
        with mrdis.hip.option('debug_volgen', 1):
            add('inputs: warp, 30 deg, zoom 0.7 (element form)', timeit(lambda: p.patch_warp(tabs['30 deg, zoom 0.7'], origins, M, shape, patch), a.reps))
            add('targets: warp, 30 deg, zoom 0.7 (element form)', timeit(lambda: p.patch_warp(tabs['30 deg, zoom 0.7'], origins, M, shape, patch, **tg), a.reps))
        add('inputs: patch_gather', timeit(lambda: p.patch_gather(tabs['no row warped'], origins, M, shape, patch), a.reps))
        add('targets: patch_gather', timeit(lambda: p.patch_gather(tabs['no row warped'], origins, M, shape, patch, **tg), a.reps))
        add('inputs: store-only', timeit(lambda: mrdis.hip.stream_fill(in_buf), a.reps))
        add('targets: store-only', timeit(lambda: mrdis.hip.stream_fill(tg_buf), a.reps))
        add('inputs + targets: torch composition', timeit(lambda: torch_batch(store, ds, with_warp(True, 0.7), o_host, patch, mins), max(a.reps // 10, 1)))
    best = {k: min(v) for k, v in rows.items()}
    ratio = lambda k, base: round(best[k] / best[base], 2)
    emit({'metric': 'warped patch batch kernels, us per call (alternating windows)', **{k: [round(v, 1) for v in vs] for k, vs in rows.items()},
          'inputs_written_mb': round(4.0 * in_buf.numel() / 1e6, 1), 'targets_written_mb': round(4.0 * tg_buf.numel() / 1e6, 1), 'present_contrasts': present,
          'inputs_warp_over_store_only': {n: ratio(f'inputs: warp, {n} (LDS tile)', 'inputs: store-only') for n in tabs},
          'targets_warp_over_store_only': {n: ratio(f'targets: warp, {n} (LDS tile)', 'targets: store-only') for n in tabs},
          'inputs_warp_over_patch_gather': {n: ratio(f'inputs: warp, {n} (LDS tile)', 'inputs: patch_gather') for n in tabs},
          'targets_warp_over_patch_gather': {n: ratio(f'targets: warp, {n} (LDS tile)', 'targets: patch_gather') for n in tabs},
          'torch_composition_over_warp': round(best['inputs + targets: torch composition']
                                               / (best['inputs: warp, 30 deg, zoom 0.7 (LDS tile)'] + best['targets: warp, 30 deg, zoom 0.7 (LDS tile)']), 1),
          'note': 'best window for the ratios'})
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
    for name in ('fixed batch', 'warping loader in the loop') * 2:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            b = b0 if name == 'fixed batch' else next(it)
            loss = step(b['inputs'], b['targets'])
        torch.cuda.synchronize()
        res.setdefault(name, []).append(round((time.perf_counter() - t0) / a.steps * 1e3, 2))
    emit({'metric': 'NVNet3D train step, ms (two alternating windows each)', 'fixed_batch': res['fixed batch'], 'warping_loader_in_loop': res['warping loader in the loop'],
          'patch_warp': 1.0, 'steps_per_window': a.steps, 'init_channels': a.channels, 'loss': float(loss.detach())})
    finish(a, lines)


def finish(a, lines):
    if a.out:
        with open(a.out, 'w') as f:
            f.write('# python tools/bench_warp.py ' + ' '.join(sys.argv[1:]) + '\n' + '\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
