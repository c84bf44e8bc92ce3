"""Time the connected-component kernels (csrc/mrdis_cc.hip: hip.cc_label, hip.cc_clean) behind mrdis.components3d / mrdis.clean_labels on one
MI355X against a store-only pass over the same bytes -- all in ONE run.
    python tools/bench_postproc.py [--out profiles/postproc_bench.txt] [--windows 3] [--iters 5] [--vol 240 240 155] [--batch 4]
Geometry: B 4 label volumes of 240 x 240 x 155: the nested ellipsoid tumours of tools/bench_surfdist.py (labels 2 / 1 / 4 from the outside in),
two more small blobs per subject and a sprinkling of specks (one voxel in 5,000, a random label), as a net's raw prediction looks.
Every GPU step is a child process of its own under its own time limit (--step-timeout); the parent never opens the GPU, writes the file after
every step and stops at the first step that fails or runs out of time.
  passes   device time of each labelling launch and each launch of the rules, from torch.profiler's device timeline (one call each)
  calls    components3d, clean_labels (defaults that remove specks and apply the ET rule) and store_only in alternating windows of `iters`
           calls bracketed by device events; every window is printed (the spread)
  scipy    one subject the other way: D2H copy, scipy.ndimage.label on the CPU, H2D copy of its int32 labels (skipped where scipy is absent)
Bytes are what the algorithm needs, N = B H W D voxels:
  cc_label   local: labels N read, parents 4 N and sizes 4 N written; merge: parents of the tile faces read (with 4 x 4 x 64 tiles nearly all:
             4 N); compress: 4 N read, the few changed parents and one count per root written                                    = 17 N
  cc_clean   scan: comp 4 N read; keep: labels N and comp 4 N read, cleaned N written; ET rule: N read where it applies           = 11 N
store_only = mrdis_stream_fill over a buffer of the bytes of components3d + clean_labels's rules."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = ('passes', 'calls', 'scipy')
LABEL_PASSES = {'local': ('cc_local_kernel',), 'merge': ('cc_merge_kernel',), 'compress': ('cc_compress_kernel',)}
CLEAN_PASSES = {'clear': ('cc_clear_kernel',), 'scan': ('cc_scan_kernel',), 'keep': ('cc_keep_kernel',), 'et': ('cc_et_kernel',)}
CLEAN_KW = dict(min_voxels=50, et_min_voxels=10 ** 7)


def volumes(B, H, W, D, seed=1):
    from bench_surfdist import ellipsoids
    rng = np.random.RandomState(seed)
    v = ellipsoids(B, H, W, D, seed, True)
    h, w, d = np.ogrid[:H, :W, :D]
    for b in range(B):
        for _ in range(2):                                           # two small blobs away from the tumour
            c = np.array([H, W, D]) * (0.1 + 0.15 * rng.rand(3))
            r = 2.0 + 4.0 * rng.rand()
            v[b][(h - c[0]) ** 2 + (w - c[1]) ** 2 + (d - c[2]) ** 2 < r * r] = 2
    specks = rng.rand(B, H, W, D) < 2e-4
    v[specks] = rng.choice(np.array([1, 2, 4], np.uint8), size=int(specks.sum()))
    return v


def step(args):
    import torch
    import mrdis
    from bench_surfdist import alternate, kernel_split, med
    dev = torch.device('cuda:0')
    hip = mrdis.hip
    H, W, D = args.vol
    B = args.batch
    N = B * H * W * D
    labels = torch.from_numpy(volumes(B, H, W, D)).to(dev)
    fg = mrdis.postproc.fg_mask((1, 2, 4))
    comp, size = hip.cc_label(labels, fg, 26)
    _, stats = mrdis.clean_labels(labels, **CLEAN_KW)
    cfg = f'B {B}, {H} x {W} x {D}, c 26; stats per sample [components, kept, foreground, removed, et_voxels, et_replaced] {stats.tolist()}'
    if args.step == 'passes':
        lab = kernel_split(lambda: hip.cc_label(labels, fg, 26), LABEL_PASSES)
        cln = kernel_split(lambda: hip.cc_clean(labels, comp, size, CLEAN_KW['min_voxels'], False, 4, CLEAN_KW['et_min_voxels'], 1), CLEAN_PASSES)
        print(json.dumps({'metric': 'device time of every launch of one call, us (torch.profiler)', 'config': cfg, 'cc_label_passes_us': lab,
                          'cc_clean_passes_us': cln}), flush=True)
        for c in (6, 18):
            print(json.dumps({'metric': f'the same for connectivity {c}', 'cc_label_passes_us': kernel_split(lambda: hip.cc_label(labels, fg, c), LABEL_PASSES)}),
                  flush=True)
    elif args.step == 'calls':
        moved = {'components3d': 17.0 * N, 'clean_labels': 28.0 * N}
        buf = torch.empty(int(moved['clean_labels']) // 16 * 4, device=dev)
        t = alternate({'components3d': lambda: mrdis.components3d(labels), 'clean_labels': lambda: mrdis.clean_labels(labels, **CLEAN_KW),
                       'store_only': lambda: hip.stream_fill(buf)}, args.windows, args.iters)
        r = {'metric': f'us per call ({args.windows} alternating windows of {args.iters} calls, incl. allocating the outputs); clean_labels = labelling + rules',
             'config': cfg, **t, 'moved_mb': {k: round(v / 1e6, 1) for k, v in moved.items()},
             'tb_per_s': {k: round(v / med(t[k]) / 1e6, 3) for k, v in moved.items()}, 'store_only_mb': round(moved['clean_labels'] / 1e6, 1),
             'clean_labels_over_store_only': round(med(t['clean_labels']) / med(t['store_only']), 2),
             'beside': 'README: 90 ms per predict_volumes batch of this geometry, 7.5 ms per region_scores batch'}
        print(json.dumps(r), flush=True)
    elif args.step == 'scipy':
        try:
            from scipy import ndimage
        except ImportError:
            print(json.dumps({'metric': 'scipy route', 'skipped': 'scipy is not importable here'}), flush=True)
            return
        structure = ndimage.generate_binary_structure(3, 3)
        one = labels[0]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = one.cpu().numpy()
        t1 = time.perf_counter()
        lab, n = ndimage.label(host > 0, structure=structure)
        t2 = time.perf_counter()
        back = torch.from_numpy(lab.astype(np.int32)).to(dev)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        del back
        print(json.dumps({'metric': 'ONE subject through the CPU: D2H copy, scipy.ndimage.label (26-connected), H2D copy of its int32 labels, ms',
                          'd2h_ms': round((t1 - t0) * 1e3, 2), 'scipy_label_ms': round((t2 - t1) * 1e3, 2), 'h2d_ms': round((t3 - t2) * 1e3, 2),
                          'total_ms': round((t3 - t0) * 1e3, 2), 'components': int(n), 'per_batch': f'x {B} subjects'}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join('profiles', 'postproc_bench.txt'))
    ap.add_argument('--windows', type=int, default=3)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--vol', type=int, nargs=3, default=[240, 240, 155])
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--step', choices=STEPS, help='run one step in this process (what the parent starts)')
    ap.add_argument('--step-timeout', type=int, default=150, help='time limit of every step, seconds')
    args = ap.parse_args()
    if args.step:
        return step(args)
    lines = [f'# Connected components and label clean-up (csrc/mrdis_cc.hip) on one MI355X; tools/bench_postproc.py --windows {args.windows} '
             f'--iters {args.iters}, one run, every step a process of its own.', '# See the tool\'s docstring for what the bytes and store_only are.']

    def dump():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')

    for name in STEPS:
        cmd = [sys.executable, os.path.abspath(__file__), '--step', name, '--windows', str(args.windows), '--iters', str(args.iters), '--batch',
               str(args.batch), '--vol'] + [str(x) for x in args.vol]
        try:
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            lines.append(json.dumps({'step': name, 'failed': f'no result within {args.step_timeout} s; the later steps were not started'}))
            dump()
            return 1
        got = [l for l in res.stdout.splitlines() if l.startswith('{')]
        lines += got
        print('\n'.join(got), flush=True)
        if res.returncode != 0:
            lines.append(json.dumps({'step': name, 'failed': f'exit status {res.returncode}; the later steps were not started',
                                     'stderr': res.stderr[-400:]}))
            dump()
            print(res.stderr[-2000:], file=sys.stderr)
            return 1
        dump()
    return 0


if __name__ == '__main__':
    sys.exit(main())
