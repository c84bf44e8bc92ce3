"""Time the two kernels of the tile-wise prediction (csrc/mrdis_segvol.hip: tilepred.tile_accum, tilepred.tile_label_volume) on one MI355X against a
store-only pass over the same bytes, against the sliding-window kernels (hip.seg_accum, hip.seg_label_volume) on equal bytes and against the torch
composition they replace, and one batch end to end -- all in ONE run.
    python tools/bench_tilepred.py [--out profiles/tilepred_bench.txt] [--windows 3] [--iters 20] [--no-batch]
Geometry: B 4, C 3, store 160 x 192 x 155, tile 128^3, Gaussian weights of sigma 0.125; the timed tile sits at origin (32, 64, 27), where the runs
of a tile column are 16-byte aligned in one acc column of four.
Each figure: warm-up, then `windows` alternating windows of `iters` calls bracketed by device events; every window is printed (the spread).
Bytes are what the algorithm needs: tile_accum = the logits read + the tile's part of acc read and written (the weight vectors are 1.5 KB);
tile_label_volume = acc read + ground truth read + labels written (incl. zeroing the counts).  store_only = mrdis_stream_fill over a buffer of the same
bytes.  seg_accum runs at 128 x 128 planes, Dz 128, D 155, z0 27: the same bytes in the same run shape; seg_label_volume on the same acc.
torch = the composition a user would write: sigmoid, flip, weight volume product, slice += (tile_accum); divide by the denominator volume, compare,
max / argmax, where, relabel, three masked sums per channel (tile_label_volume).
End to end: predict_tiles over one batch of four subjects, NVNet3D with init_channels 16 and random weights, stride = tile / 2 (2 x 2 x 2 tiles),
without mirroring and with mirror 'hwd' (8 and 64 forwards), beside predict_volumes on the same batch (depth window 128 over the full 160 x 192
planes, stride 64: 2 forwards); a host clock around the whole generator, ended by a device synchronise."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mrdis  # noqa: E402

B, C, H, W, D, TT = 4, 3, 160, 192, 155, 128
ORIGIN = (32, 64, 27)
CONTRASTS = ['T1', 'T1c', 'T2', 'T2_FLAIR']


def window_us(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return round(a.elapsed_time(b) * 1e3 / iters, 1)


def alternate(fns, windows, iters):
    """{name: [us per call of each window]}: the candidates take turns inside every window"""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            out[k].append(window_us(fn, iters))
    return out


def med(v):
    return float(np.median(v))


def torch_accum(logits, acc, w3, origin, dims):
    p = torch.sigmoid(logits.permute(0, 2, 3, 4, 1))
    if dims:
        p = p.flip(dims)
    h0, w0, d0 = origin
    acc[:, h0:h0 + TT, w0:w0 + TT, d0:d0 + TT] += w3 * p


def torch_labels(acc, den, tv, relabel=True):
    pbar = torch.where(den > 0, acc / den, torch.zeros_like(acc))
    pred = pbar > 0.5
    mx, arg = pbar.max(-1)
    lab = torch.where(mx > 0.5, arg + 1, torch.zeros_like(arg))
    t = tv
    if relabel:
        lab = torch.where(lab == 3, torch.full_like(lab, 4), lab)
        t = torch.where(tv == 4, torch.full_like(tv, 3), tv)
    counts = torch.stack([torch.stack([(pred[..., c] & (t == c + 1)).sum((1, 2, 3)), pred[..., c].sum((1, 2, 3)), (t == c + 1).sum((1, 2, 3))], -1)
                          for c in range(C)], 1)
    return lab.to(torch.uint8), counts.int()


def timed_batch(gen_fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for r in gen_fn():
        del r
    torch.cuda.synchronize()
    return round((time.perf_counter() - t0) * 1e3, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join('profiles', 'tilepred_bench.txt'))
    ap.add_argument('--windows', type=int, default=3)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--no-batch', action='store_true')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    hip, tp = mrdis.hip, mrdis.tilepred
    torch.manual_seed(0)
    recs = []
    cfg = f'B {B}, C {C}, store {H} x {W} x {D}, tile {TT}^3 at {ORIGIN}'
    # ---- tile_accum
    logits = (3 * torch.randn(B, TT, TT, TT, C, device=dev)).permute(0, 4, 1, 2, 3)
    wv = tuple(torch.from_numpy(mrdis.tile_weights(TT)).to(dev) for _ in range(3))
    w3 = ((wv[0][:, None] * wv[1][None, :])[:, :, None] * wv[2][None, None, :])[None, ..., None]
    acc = torch.zeros(B, H, W, D, C, device=dev)
    acc_t = torch.zeros_like(acc)
    differ = {}
    for name, flips, dims in (('plain', 0, []), ('d_mirrored', 8, [3]), ('hwd_mirrored', 13, [1, 2, 3])):
        acc.zero_(); acc_t.zero_()
        tp.tile_accum(logits, acc, wv, ORIGIN, flips)
        torch_accum(logits, acc_t, w3, ORIGIN, dims)
        differ[name] = float((acc - acc_t).abs().max())
    sacc = torch.zeros(B, TT, TT, D, C, device=dev)                                                # seg_accum on equal bytes
    ones = tuple(torch.ones(TT, device=dev) for _ in range(3))
    nbytes = 3 * B * C * TT ** 3 * 4
    fill_buf = torch.empty(nbytes // 4, device=dev)
    t = alternate({'kernel_plain': lambda: tp.tile_accum(logits, acc, wv, ORIGIN, 0),
                   'kernel_d_mirrored': lambda: tp.tile_accum(logits, acc, wv, ORIGIN, 8),
                   'kernel_hwd_mirrored': lambda: tp.tile_accum(logits, acc, wv, ORIGIN, 13),
                   'kernel_plain_uniform': lambda: tp.tile_accum(logits, acc, ones, ORIGIN, 0),
                   'seg_accum_equal_bytes': lambda: hip.seg_accum(logits, sacc, ORIGIN[2]),
                   'torch_plain': lambda: torch_accum(logits, acc_t, w3, ORIGIN, []),
                   'torch_d_mirrored': lambda: torch_accum(logits, acc_t, w3, ORIGIN, [3]),
                   'store_only': lambda: hip.stream_fill(fill_buf)}, args.windows, args.iters)
    recs.append({'metric': f'mrdis_tile_accum, us per tile and view ({args.windows} alternating windows)', 'config': cfg, **t,
                 'moved_mb': round(nbytes / 1e6, 1), 'note': 'moved = logits read + acc tile read + acc tile write',
                 'tb_per_s': {k: round(nbytes / med(v) / 1e6, 2) for k, v in t.items() if k.startswith(('kernel', 'seg_accum', 'store'))},
                 'kernel_over_store_only': {k: round(med(v) / med(t['store_only']), 2) for k, v in t.items() if k.startswith('kernel')},
                 'kernel_over_seg_accum': round(med(t['kernel_plain']) / med(t['seg_accum_equal_bytes']), 2),
                 'torch_over_kernel': {'plain': round(med(t['torch_plain']) / med(t['kernel_plain']), 2),
                                       'd_mirrored': round(med(t['torch_d_mirrored']) / med(t['kernel_d_mirrored']), 2)},
                 'max_abs_difference_from_torch_one_call': differ})
    print(json.dumps(recs[-1]), flush=True)
    del fill_buf, sacc, acc_t, logits, w3
    # ---- tile_label_volume
    offs = mrdis.tile_offsets((H, W, D), (TT, TT, TT))
    wn = [mrdis.tile_weights(TT)] * 3
    norms = tuple(torch.from_numpy(mrdis.tile_norm(n, TT, o, w)).to(dev) for n, o, w in zip((H, W, D), offs, wn))
    den = ((norms[0][:, None] * norms[1][None, :])[:, :, None] * norms[2][None, None, :])[None, ..., None]
    acc = (torch.rand(B, H, W, D, C, device=dev) * den).contiguous()                                # pbar uniform in 0 .. 1
    tvol = [torch.randint(0, 5, (H, W, D), device=dev).float() for _ in range(B)]
    tvol = [torch.where(v == 3, torch.full_like(v, 4.0), v) for v in tvol]
    ptrs = torch.tensor([v.data_ptr() for v in tvol], dtype=torch.int64).to(dev)
    tv = torch.stack(tvol)
    cover = torch.from_numpy(mrdis.model3d.window_cover(D, TT, offs[2])).to(dev)
    lab_k, cnt_k = tp.tile_label_volume(acc, norms, ptrs, relabel=True)
    lab_t, cnt_t = torch_labels(acc, den, tv)
    nbytes = B * H * W * D * (C * 4 + 4 + 1)
    fill_buf = torch.empty(nbytes // 16 * 4, device=dev)
    t = alternate({'kernel': lambda: tp.tile_label_volume(acc, norms, ptrs, relabel=True),
                   'seg_label_volume': lambda: hip.seg_label_volume(acc, cover, ptrs, relabel=True),
                   'torch': lambda: torch_labels(acc, den, tv),
                   'store_only': lambda: hip.stream_fill(fill_buf)}, args.windows, args.iters)
    recs.append({'metric': f'mrdis_tile_label_volume (incl. zeroing the counts), us per call ({args.windows} alternating windows)', 'config': cfg, **t,
                 'moved_mb': round(nbytes / 1e6, 1), 'note': 'moved = acc read + ground truth read + labels written',
                 'tb_per_s': round(nbytes / med(t['kernel']) / 1e6, 2), 'seg_label_volume_tb_per_s': round(nbytes / med(t['seg_label_volume']) / 1e6, 2),
                 'store_only_tb_per_s': round(nbytes / med(t['store_only']) / 1e6, 2),
                 'kernel_over_store_only': round(med(t['kernel']) / med(t['store_only']), 2),
                 'kernel_over_seg_label_volume': round(med(t['kernel']) / med(t['seg_label_volume']), 2),
                 'torch_over_kernel': round(med(t['torch']) / med(t['kernel']), 2),
                 'labels_differ_from_torch': int((lab_k != lab_t).sum()), 'counts_equal_torch': bool(torch.equal(cnt_k, cnt_t))})
    print(json.dumps(recs[-1]), flush=True)
    del fill_buf, acc, den, tv, tvol, lab_k, lab_t
    torch.cuda.empty_cache()
    # ---- one batch end to end
    if not args.no_batch:
        g = np.random.RandomState(1)
        arrays = {}
        for s in range(B):
            for c in CONTRASTS:
                arrays[f'S{s}/{c}'] = g.randn(H, W, D).astype(np.float32)
            arrays[f'S{s}/seg'] = g.randint(0, 3, (H, W, D)).astype(np.float32)
        store = mrdis.VolumeStore3D.from_arrays(arrays, dev)
        ds = mrdis.VolumeDataset3D('BraTS', store, [f'S{s}' for s in range(B)], CONTRASTS, patch_size=(TT, TT, TT), patch_centre=True)
        loader = mrdis.VolumeLoader3D(ds, B, region_channels=3)
        torch.manual_seed(10)
        model = mrdis.NVNet3D((TT, TT, TT), 4, 3, 16).to(dev)
        runs = {'predict_tiles_ms': lambda: mrdis.predict_tiles(model, loader, (TT, TT, TT)),
                'predict_tiles_mirror_hwd_ms': lambda: mrdis.predict_tiles(model, loader, (TT, TT, TT), mirror='hwd'),
                'predict_volumes_ms': lambda: mrdis.predict_volumes(model, loader)}
        ms = {k: [] for k in runs}
        hip.launch_counts(reset=True)
        timed_batch(runs['predict_tiles_ms'])
        lc = hip.launch_counts()
        timed_batch(runs['predict_volumes_ms'])
        for _ in range(args.windows):
            for k, fn in runs.items():
                ms[k].append(timed_batch(fn))
        recs.append({'metric': f'one batch end to end, ms per batch ({args.windows} alternating runs after a warm-up)',
                     'config': f'B {B}, {H} x {W} x {D}, M 4, NVNet3D init_channels 16, random weights; tiles {TT}^3 at stride {TT // 2}: '
                               f'{[len(o) for o in offs]} tiles; predict_volumes: depth window {TT}, stride {TT // 2}, '
                               f'{len(mrdis.window_offsets(D, TT, TT // 2))} windows of {H} x {W} x {TT}', **ms,
                     'tileaccum_launches_no_mirror': lc['tileaccum'], 'tilelabels_launches': lc['tilelabels'],
                     'ms_per_forward': {'predict_tiles': round(med(ms['predict_tiles_ms']) / 8, 1),
                                        'predict_tiles_mirror_hwd': round(med(ms['predict_tiles_mirror_hwd_ms']) / 64, 1),
                                        'predict_volumes': round(med(ms['predict_volumes_ms']) / len(mrdis.window_offsets(D, TT, TT // 2)), 1)}})
        print(json.dumps(recs[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(f'# Tile-wise prediction (csrc/mrdis_segvol.hip: mrdis_tile_accum, mrdis_tile_label_volume) on {torch.cuda.get_device_name(dev)}, fp32; '
                f'tools/bench_tilepred.py --windows {args.windows} --iters {args.iters}, one process, one run.\n'
                f'# See the tool\'s docstring for what the bytes, store_only, seg_accum / seg_label_volume and torch rows are.\n')
        for r in recs:
            f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
