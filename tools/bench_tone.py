"""Timing of the intensity augmentation of the 3-D training patches (csrc/mrdis_tone.hip, tone3d.py, data3d.py's `patch_blur` .. `patch_noise_std`
keys) on one MI355X:

    python tools/bench_tone.py [--batch 4] [--patch 128 128 128] [--out profiles/tone_bench.txt]

Times, in alternating windows inside ONE run (the repeats give the box's spread), each of the three calls -- mrdis_patch_blur, mrdis_patch_stats,
mrdis_patch_tone -- on a (B, 4, PH, PW, PD) batch with 30 % background: with every row flagged (blur at sigma 1.0; contrast, gamma and noise
together), with no row flagged, in the generic form (debug_volgen) with every row flagged; a store-only pass over the same bytes
(mrdis_stream_fill); and the torch composition of the same step (a masked F.conv3d per axis; amin / amax / mean; clamp, pow and randn).  Then
the NVNet3D step on a fixed batch against the same step with the intensifying loader in the loop (the synthetic BraTS-shaped store of
tools/bench_patch.py).  One JSON line per result; with --out the lines are also written to that file.  No threshold: the numbers are
recorded as they come out.
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
from bench_patch import CONTRASTS, build_store, timeit  # noqa: E402

t3 = mrdis.tone3d
ALL = t3.BLUR | t3.CONTRAST | t3.GAMMA | t3.NOISE


def torch_blur(x, g):
    """the blur as the obvious torch composition: x (B, M, PH, PW, PD), g (M, 9) full taps -> the masked, renormalised separable convolution"""
    M = x.shape[1]
    m = (x != -10).float()
    n, d = x * m, m
    for axis in (4, 3, 2):
        shape = [M, 1, 1, 1, 1]
        shape[axis] = 9
        pad = [0, 0, 0]
        pad[axis - 2] = 4
        w = g.reshape(shape)
        n, d = F.conv3d(n, w, padding=pad, groups=M), F.conv3d(d, w, padding=pad, groups=M)
    return torch.where(m > 0, n / d.clamp_min(1e-30), x)


def torch_stats(y):
    m = y != -10
    big = torch.finfo(y.dtype).max
    lo = torch.where(m, y, torch.full_like(y, big)).amin(dim=(2, 3, 4))
    hi = torch.where(m, y, torch.full_like(y, -big)).amax(dim=(2, 3, 4))
    n = m.sum(dim=(2, 3, 4))
    mean = (torch.where(m, y, torch.zeros_like(y)).sum(dim=(2, 3, 4), dtype=torch.float64) / n.clamp_min(1)).float()
    return lo, hi, mean, n


def torch_tone(y, st, f, gamma, std):
    lo, hi, mean, _ = (v[:, :, None, None, None] for v in st)
    e = lambda v: v[None, :, None, None, None]
    m = y != -10
    v = torch.minimum(torch.maximum(mean + (y - mean) * e(f), lo), hi)
    rg = (hi - lo).clamp_min(1e-30)
    v = lo + ((v - lo) / rg).clamp(0, 1).pow(e(gamma)) * rg
    v = v + e(std) * torch.randn_like(v)
    return torch.where(m, v, y)


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
    patch = tuple(a.patch)
    PH, PW, PD = patch
    B, M = a.batch, 4
    lines = []

    def emit(row):
        row['config'] = f'B={B} M={M} patch {PH}x{PW}x{PD} fp32'
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    torch.manual_seed(1)
    x = torch.randn((B, PH, PW, PD, M), device=dev)
    x[torch.rand_like(x) < 0.3] = -10.0
    x = x.permute(0, 4, 1, 2, 3)
    col = 2 * M + 7
    rs = np.random.RandomState(1)

    def table(flags, sigma=1.0):
        tab = np.zeros((B, col + t3.TONE_EXTRA(M)), dtype=np.int64)
        for b in range(B):
            tab[b, col:] = t3.pack_tone(rs.randint(0, 2 ** 32, size=2, dtype=np.uint32), [flags] * M, [sigma] * M, [1.2] * M, [1.4] * M, [0.1] * M)
        return torch.from_numpy(tab).to(dev)

    tabs = {'every row flagged': table(ALL), 'no row flagged': table(0)}
    y = t3.patch_blur(x, tabs['every row flagged'], col, M)
    st = t3.patch_stats(y, M)
    # sanity, not a test: the torch composition lands near the kernels
    g = torch.from_numpy(np.stack([np.concatenate([t3.blur_taps(1.0)[:0:-1], t3.blur_taps(1.0)])] * M)).to(dev)
    yt = torch_blur(x, g)
    stt = torch_stats(y)
    emit({'metric': 'torch composition against the kernels', 'blur_max_abs_difference': float((yt - y).abs().max()), 'markers_equal': bool(torch.equal(yt == -10, y == -10)),
          'lo_hi_n_equal': bool(torch.equal(stt[0].view(torch.int32), st[:, :, 0]) and torch.equal(stt[1].view(torch.int32), st[:, :, 1]) and torch.equal(stt[3].int(), st[:, :, 3])),
          'mean_max_abs_difference': float((stt[2] - st[:, :, 2].view(torch.float32)).abs().max())})
    del yt
    f_, gm_, sd_ = (torch.full((M,), v, device=dev) for v in (1.2, 1.4, 0.1))
    buf = torch.empty(x.numel(), device=dev)
    work = y.clone()
    rows = {}
    add = lambda k, v: rows.setdefault(k, []).append(v)
    for _ in range(a.windows):
        for name, tab in tabs.items():
            add(f'blur: {name}', timeit(lambda: t3.patch_blur(x, tab, col, M), a.reps))
            add(f'tone: {name}', timeit(lambda: t3.patch_tone(work, st, tab, col, M), a.reps))
        add('stats', timeit(lambda: t3.patch_stats(y, M), a.reps))
        with mrdis.hip.option('debug_volgen', 1):
            add('blur: every row flagged (generic form)', timeit(lambda: t3.patch_blur(x, tabs['every row flagged'], col, M), max(a.reps // 5, 1)))
            add('stats (generic form)', timeit(lambda: t3.patch_stats(y, M), max(a.reps // 5, 1)))
            add('tone: every row flagged (generic form)', timeit(lambda: t3.patch_tone(work, st, tabs['every row flagged'], col, M), max(a.reps // 5, 1)))
        add('store-only', timeit(lambda: mrdis.hip.stream_fill(buf), a.reps))
        add('blur: torch composition', timeit(lambda: torch_blur(x, g), max(a.reps // 10, 1)))
        add('stats: torch composition', timeit(lambda: torch_stats(y), max(a.reps // 10, 1)))
        add('tone: torch composition', timeit(lambda: torch_tone(y, stt, f_, gm_, sd_), max(a.reps // 10, 1)))
    best = {k: min(v) for k, v in rows.items()}
    over = lambda k, base='store-only': round(best[k] / best[base], 2)
    emit({'metric': 'intensity kernels, us per call (alternating windows)', **{k: [round(v, 1) for v in vs] for k, vs in rows.items()},
          'bytes_mb': round(4.0 * x.numel() / 1e6, 1),
          'over_store_only': {k: over(k) for k in ('blur: every row flagged', 'blur: no row flagged', 'stats', 'tone: every row flagged', 'tone: no row flagged')},
          'torch_over_kernel': {'blur': over('blur: torch composition', 'blur: every row flagged'), 'stats': over('stats: torch composition', 'stats'),
                                'tone': over('tone: torch composition', 'tone: every row flagged')},
          'note': 'best window for the ratios'})
    del buf, work, y
    if a.steps < 1:
        return finish(a, lines)

    H, W, D = a.vol
    nsubj = 8
    store = build_store(dev, H, W, D, nsubj)
    ds = mrdis.VolumeDataset3D('BraTS', store, [f's{s:02d}' for s in range(nsubj)], CONTRASTS, aug=True, dropoff=True)
    loader = mrdis.VolumeLoader3D(ds, B, shuffle=True, region_channels=3, patch_size=patch, patch_fg=0.33, patch_flips='hwd', patch_blur=1.0, patch_contrast=1.0,
                                  patch_gamma=1.0, patch_noise=1.0)
    np.random.seed(1); torch.manual_seed(10)
    model = mrdis.NVNet3D(patch, M, 3, a.channels, p=0.2).to(dev).train()
    opt = mrdis.ArenaAdam(model.parameters(), lr=1e-4, weight_decay=1e-5)

    def step(xb, tb):
        loss, _ = mrdis.nvnet_loss_hip(*model(xb), xb, tb)
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
    for name in ('fixed batch', 'intensifying loader in the loop') * 2:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            b = b0 if name == 'fixed batch' else next(it)
            loss = step(b['inputs'], b['targets'])
        torch.cuda.synchronize()
        res.setdefault(name, []).append(round((time.perf_counter() - t0) / a.steps * 1e3, 2))
    emit({'metric': 'NVNet3D train step, ms (two alternating windows each)', 'fixed_batch': res['fixed batch'], 'intensifying_loader_in_loop': res['intensifying loader in the loop'],
          'shares': 1.0, 'store': f'{H}x{W}x{D}', 'steps_per_window': a.steps, 'init_channels': a.channels, 'loss': float(loss.detach())})
    finish(a, lines)


def finish(a, lines):
    if a.out:
        with open(a.out, 'w') as f:
            f.write('# python tools/bench_tone.py ' + ' '.join(sys.argv[1:]) + '\n' + '\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
