"""Time the region-scoring kernels (csrc/mrdis_surfdist.hip: hip.region_surfaces, hip.edt_sq, hip.surface_hist) and mrdis.region_scores on one
MI355X against a store-only pass over the same bytes -- all in ONE run.
    python tools/bench_surfdist.py [--out profiles/surfdist_bench.txt] [--windows 3] [--iters 5] [--vol 240 240 155] [--batch 4]
Geometry: B 4 label volumes of 240 x 240 x 155 with synthetic nested ellipsoid tumours (labels 2 / 1 / 4 from the outside in); the prediction
is the ground truth's ellipsoid moved and rescaled a little, so Dice is about 0.8 and the surfaces are a few voxels apart, as for a good net.
Each figure: warm-up, then `windows` alternating windows of `iters` calls bracketed by device events; every window is printed (the spread).
Bytes are what the algorithm needs, N = B H W D voxels, S sources:
  region_surfaces   labels N + ground truth 4 N read, flags N written (the six neighbours of the few voxels inside a region come from cache)
  edt, pass D       flags N read, S x 2 N written (uint16 distances)
  edt, pass W       S x 2 N read, S x 4 N written
  edt, pass H       S x 4 N read, S x 4 N written; in histogram form S x 4 N read + the flags S x N read, nothing written but the histogram
A call of hip.edt_sq is the three passes, a call of hip.surface_hist (S = 2 R = 6) passes D, W and the histogram form of H; `passes_us` splits a
call into its kernels from the device timeline of torch.profiler where that is available.  store_only = mrdis_stream_fill over a buffer of the
same bytes.  region_scores is timed end to end (kernels, the torch running sums over the histograms, the one D2H copy) and beside one
predict_volumes batch of the same geometry (NVNet3D, init_channels 16, stride 32, no flip).  If scipy is importable, the CPU time of its
distance_transform_edt on one of the surfaces is recorded, for orientation only."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mrdis  # noqa: E402


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
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            out[k].append(window_us(fn, iters))
    return out


def med(v):
    return float(np.median(v))


def ellipsoids(B, H, W, D, seed, moved):
    """(B, H, W, D) uint8 nested ellipsoids: 2 outside, 1 inside it, 4 at the core"""
    rng = np.random.RandomState(seed)
    h, w, d = np.ogrid[:H, :W, :D]
    out = np.zeros((B, H, W, D), dtype=np.uint8)
    for b in range(B):
        c = np.array([H, W, D]) * (0.5 + 0.1 * rng.rand(3)) + (np.array([1.5, -1.0, 2.0]) if moved else 0.0)
        rad = np.array([H, W, D]) * (0.14 + 0.06 * rng.rand(3)) * (1.04 if moved else 1.0)
        q = ((h - c[0]) / rad[0]) ** 2 + ((w - c[1]) / rad[1]) ** 2 + ((d - c[2]) / rad[2]) ** 2
        out[b][q < 1.0] = 2
        out[b][q < 0.5] = 1
        out[b][q < 0.2] = 4
    return out


def kernel_split(fn, names):
    """{pass: device us of one call} from torch.profiler's device timeline (names: {pass: fragments of the kernel's plain or mangled name}),
    None if the profiler gives none"""
    try:
        from torch.profiler import profile, ProfilerActivity
        fn(); torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.key_averages():
            t = getattr(ev, 'device_time_total', None)
            if t is None:
                t = getattr(ev, 'cuda_time_total', 0.0)
            for n, frags in names.items():
                if t and any(f in ev.key for f in frags):
                    out[n] = round(out.get(n, 0.0) + float(t), 1)
        return out or None
    except Exception as e:          # the split is a convenience: the per-call figures do not depend on it
        return {'unavailable': repr(e)[:120]}


PASSES = {'scan_D': ('edt_scan_kernel',), 'minplus_W': ('edt_minplus_kernel<unsigned short', 'edt_minplus_kernelIt'),
          'minplus_H': ('edt_minplus_kernel<int', 'edt_minplus_kernelIi')}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join('profiles', 'surfdist_bench.txt'))
    ap.add_argument('--windows', type=int, default=3)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--vol', type=int, nargs=3, default=[240, 240, 155])
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--channels', type=int, default=16)
    ap.add_argument('--no-predict', action='store_true', help='skip the predict_volumes batch')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    hip = mrdis.hip
    H, W, D = args.vol
    B = args.batch
    N = B * H * W * D
    gt_np, pred_np = ellipsoids(B, H, W, D, 1, False), ellipsoids(B, H, W, D, 1, True)
    labels = torch.from_numpy(pred_np).to(dev)
    gts = [torch.from_numpy(g.astype(np.float32)).to(dev) for g in gt_np]
    ptrs = torch.tensor([g.data_ptr() for g in gts], dtype=torch.int64).to(dev)
    _, masks = mrdis.region_masks(mrdis.BRATS_REGIONS)
    flags, counts = hip.region_surfaces(labels, ptrs, masks)
    cfgtxt = f'B {B}, {H} x {W} x {D}, regions wt / tc / et; surface voxels of the prediction per sample and region {counts[:, :, 3].tolist()}'
    recs = []

    def dump():                     # after every record: a later stage that fails leaves the earlier figures on disk
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(f'# Region scoring (csrc/mrdis_surfdist.hip) on one MI355X (the runtime\'s device name: {torch.cuda.get_device_name(dev)}); '
                    f'tools/bench_surfdist.py --windows {args.windows} --iters {args.iters}, one process, one run.\n'
                    f'# See the tool\'s docstring for what the bytes, store_only and passes_us rows are.\n')
            for r in recs:
                f.write(json.dumps(r) + '\n')

    def fill(nbytes):
        return torch.empty(int(nbytes) // 16 * 4, device=dev)

    def record(metric, t, moved, kernel_key, extra=None):
        r = {'metric': metric, 'config': cfgtxt, **t, 'moved_mb': round(moved / 1e6, 1),
             'tb_per_s': round(moved / med(t[kernel_key]) / 1e6, 3), 'kernel_over_store_only': round(med(t[kernel_key]) / med(t['store_only']), 2)}
        r.update(extra or {})
        recs.append(r)
        print(json.dumps(r), flush=True)
        dump()

    # region surfaces
    moved = 6.0 * N
    buf = fill(moved)
    t = alternate({'kernel': lambda: hip.region_surfaces(labels, ptrs, masks), 'store_only': lambda: hip.stream_fill(buf)}, args.windows, args.iters)
    record(f'mrdis_region_surfaces (incl. allocating flags and zeroing counts), us per call ({args.windows} alternating windows)', t, moved, 'kernel')
    del buf
    # the transform alone: one source and six
    for S in (1, 6):
        bits = [1 << k for k in (0, 1, 2, 4, 5, 6)][:S]
        moved = N * (1.0 + 2 * S) + N * 6.0 * S + N * 8.0 * S
        buf = fill(moved)
        t = alternate({'kernel': lambda: hip.edt_sq(flags, bits), 'store_only': lambda: hip.stream_fill(buf)}, args.windows, args.iters)
        split = kernel_split(lambda: hip.edt_sq(flags, bits), PASSES)
        record(f'mrdis_edt_sq, S = {S} (three passes, incl. allocating the output), us per call ({args.windows} alternating windows)', t, moved, 'kernel',
               {'passes_us': split})
        del buf
    # the histogram form
    moved = N * (1.0 + 12.0) + N * 36.0 + N * (24.0 + 6.0)
    buf = fill(moved)
    t = alternate({'kernel': lambda: hip.surface_hist(flags, 3), 'store_only': lambda: hip.stream_fill(buf)}, args.windows, args.iters)
    split = kernel_split(lambda: hip.surface_hist(flags, 3), PASSES)
    record(f'mrdis_surface_hist, R = 3 (D scan, W pass, histogram pass; incl. zeroing the histogram), us per call ({args.windows} alternating windows)',
           t, moved, 'kernel', {'passes_us': split})
    del buf
    # end to end
    res = mrdis.region_scores(labels, ptrs)
    t = alternate({'region_scores': lambda: mrdis.region_scores(labels, ptrs)}, args.windows, args.iters)
    r = {'metric': f'region_scores end to end, us per batch ({args.windows} windows)', 'config': cfgtxt, **t,
         'dice': [[round(x, 4) for x in row] for row in res['dice'].tolist()], 'hd95': [[round(x, 3) for x in row] for row in res['hd95'].tolist()]}
    if not args.no_predict:
        contrasts = ['T1', 'T1c', 'T2', 'T2_FLAIR']
        g = torch.Generator().manual_seed(4)
        store = mrdis.VolumeStore3D(dev)
        for s_ in range(B):
            for c in contrasts:
                store.add(f's{s_:02d}/{c}', torch.randn(H, W, D, generator=g).numpy())
            store.add(f's{s_:02d}/seg', gt_np[s_].astype(np.float32))
        ds = mrdis.VolumeDataset3D('BraTS', store, [f's{s_:02d}' for s_ in range(B)], contrasts)
        loader = mrdis.VolumeLoader3D(ds, B, region_channels=3)
        torch.manual_seed(10)
        model = mrdis.NVNet3D((H, W, ds.crop()[1]), 4, 3, args.channels, p=0.2).to(dev)

        def whole():
            for out in mrdis.predict_volumes(model, loader, stride=32):
                last = out['labels']
            torch.cuda.synchronize()
            return last

        whole()
        ms = []
        for _ in range(args.windows):
            t0 = time.perf_counter()
            whole()
            ms.append(round((time.perf_counter() - t0) * 1e3, 1))
        r['predict_volumes_ms_per_batch'] = ms
        r['region_scores_share_of_a_predict_batch'] = round(med(t['region_scores']) / 1e3 / med(ms), 3)
        r['note'] = f'predict_volumes: NVNet3D init_channels {args.channels}, stride 32, no flip; share = region_scores / predict_volumes'
    recs.append(r)
    print(json.dumps(r), flush=True)
    dump()
    try:
        from scipy.ndimage import distance_transform_edt
        surf = ((flags[0] >> 4) & 1).cpu().numpy() == 0
        t0 = time.perf_counter()
        distance_transform_edt(surf)
        r = {'metric': 'scipy.ndimage.distance_transform_edt on the CPU, one surface of one subject, s (orientation only)',
             'seconds': round(time.perf_counter() - t0, 2), 'transforms_per_batch': 6 * B}
        recs.append(r)
        print(json.dumps(r), flush=True)
    except ImportError:
        pass
    dump()


if __name__ == '__main__':
    main()
