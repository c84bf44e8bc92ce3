"""Time the lesion-wise scoring (csrc/mrdis_lesion.hip behind mrdis.dilate3d / mrdis.lesion_scores) on one MI355X against a store-only pass over
the same bytes and against the CPU route -- all in ONE run.
    python tools/bench_lesion.py [--out profiles/lesion_bench.txt] [--windows 3] [--iters 5] [--vol 240 240 155] [--batch 4]
Geometry: B 4 label volumes of 240 x 240 x 155.  The prediction is the volume of tools/bench_postproc.py: nested ellipsoid tumours (labels 2 / 1 / 4
from the outside in), two more small blobs per subject and a sprinkling of specks (one voxel in 5,000), as a net's raw prediction looks.  The
ground truth is the same scene before the tumour moved, with its own two small blobs and without specks.
Every GPU step is a child process of its own under its own time limit (--step-timeout); the parent never opens the GPU, writes the file after
every step and stops at the first step that fails or runs out of time.
  kernels  each new kernel beside a store-only pass (mrdis_stream_fill) over the bytes it needs, in alternating windows of `iters` calls bracketed
           by device events.  N = B H W D voxels, R = 3 regions, n = the lesions of a chunk:
             region_planes   labels N and fp32 ground truth 4 N read, planes N written                                        =  6 N
             dilate x 3      per iteration N read (the halo comes from LDS and the caches) and N written                      =  6 N
             lesion_match    per item comp_l 4 and comp_p 4 read, planes 1; the gathers at roots stay in cache                = 27 N  (9 R N)
             lesion_expand   per lesion comp_l 4, comp_p 4 and planes 1 read, two masks written                               = 11 n N / B
  scores   lesion_scores per batch end to end, and its parts in the same windows: the labelling (planes, dilation, two cc_label calls and the
           running sums), the matching, and the per-lesion scoring (expand + crop + region_surfaces + surface_hist per chunk of max_items
           lesions), each of the last two also on the whole volume (crop=False: the same bits)
  cpu      one subject the other way: D2H copy, scipy binary_dilation x 3 + label of one region, and one distance transform of one lesion mask"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
STEPS = ('kernels', 'scores', 'cpu')


def volumes(B, H, W, D):
    """(prediction, ground truth), both (B, H, W, D) uint8"""
    from bench_postproc import volumes as predicted
    from bench_surfdist import ellipsoids
    rng = np.random.RandomState(2)
    truth = ellipsoids(B, H, W, D, 1, False)
    h, w, d = np.ogrid[:H, :W, :D]
    for b in range(B):
        for _ in range(2):                                           # two small lesions away from the tumour, one of them missed
            c = np.array([H, W, D]) * (0.75 + 0.1 * rng.rand(3))
            r = 3.0 + 3.0 * rng.rand()
            truth[b][(h - c[0]) ** 2 + (w - c[1]) ** 2 + (d - c[2]) ** 2 < r * r] = 2
    return predicted(B, H, W, D), truth


def step(args):
    import torch
    import mrdis
    from bench_surfdist import alternate, med
    dev = torch.device('cuda:0')
    hip, les = mrdis.hip, mrdis.lesion
    H, W, D = args.vol
    B, R = args.batch, 3
    N = B * H * W * D
    pred, truth = volumes(B, H, W, D)
    labels = torch.from_numpy(pred).to(dev)
    target = torch.from_numpy(truth).to(dev).float()
    table = torch.tensor([target.data_ptr() + b * H * W * D * 4 for b in range(B)], dtype=torch.int64).to(dev)
    _, masks = mrdis.region_masks(mrdis.BRATS_REGIONS)
    res = mrdis.lesion_scores(labels, table)
    cfg = (f'B {B}, {H} x {W} x {D}, dilation 3, min_voxels 50, max_items 8; counts per sample and region [lesions, kept, missed, components, fp] '
           f'{res["counts"].tolist()}; lesion_dice {[[round(v, 4) for v in r] for r in res["lesion_dice"].tolist()]}')
    n_les = int(res['lesions'].shape[0])

    def fill(nbytes):
        buf = torch.empty(max(4, int(nbytes) // 16 * 4), device=dev)
        return lambda: hip.stream_fill(buf)

    def label_part():
        planes = les.region_planes(labels, table, masks)
        grown = les.dilate(planes, 3, 18)
        shifts = torch.arange(R, dtype=torch.uint8, device=dev).view(1, R, 1, 1, 1)
        comp_p, size_p = hip.cc_label(((planes.unsqueeze(1) >> shifts) & 1).view(B * R, H, W, D), 2, 26)
        comp_l, size_l = hip.cc_label(((grown.unsqueeze(1) >> (shifts + 4)) & 1).view(B * R, H, W, D), 2, 26)
        rank_p = (torch.cumsum((size_p > 0).view(-1), 0, dtype=torch.int32) - 1).view(B * R, H, W, D)
        rank_l = (torch.cumsum((size_l > 0).view(-1), 0, dtype=torch.int32) - 1).view(B * R, H, W, D)
        return planes, comp_l, rank_l, comp_p, rank_p

    planes, comp_l, rank_l, comp_p, rank_p = label_part()
    ends = torch.arange(1, B * R + 1, device=dev) * (H * W * D) - 1
    cum_p = (rank_p.view(-1)[ends] + 1).cpu().numpy()
    first_p = torch.from_numpy(np.concatenate([[0], cum_p[:-1]]).astype(np.int32)).to(dev)
    words = max(1, (int(np.diff(cum_p, prepend=0).max()) + 31) // 32)
    ops = (planes, comp_l, rank_l, comp_p, rank_p, first_p, R)
    bits, tcount, root, item = les.lesion_match(*ops, n_les, words)
    n = min(8, n_les)
    if args.step == 'kernels':
        moved = {'region_planes': 6.0 * N, 'dilate3': 6.0 * N, 'lesion_match': 27.0 * N, 'lesion_expand': 11.0 * n * N / B}
        fns = {'region_planes': lambda: les.region_planes(labels, table, masks), 'dilate3': lambda: les.dilate(planes, 3, 18),
               'lesion_match': lambda: les.lesion_match(*ops, n_les, words), 'lesion_expand': lambda: les.lesion_expand(*ops, bits, item, 0, n)}
        for k in list(fns):
            fns['store_' + k] = fill(moved[k])
        t = alternate(fns, args.windows, args.iters)
        print(json.dumps({'metric': f'us per call ({args.windows} alternating windows of {args.iters} calls, incl. allocating the outputs); store_X = a store-only pass '
                                    f'over the bytes of X; lesion_expand for a chunk of {n} lesions', 'config': cfg, **t,
                          'moved_mb': {k: round(v / 1e6, 1) for k, v in moved.items()},
                          'tb_per_s': {k: round(v / med(t[k]) / 1e6, 3) for k, v in moved.items()},
                          'over_store_only': {k: round(med(t[k]) / med(t['store_' + k]), 2) for k in moved}, 'match_words': words}), flush=True)
    elif args.step == 'scores':
        boxes = []

        def chunks(crop=True):
            del boxes[:]
            for j0 in range(0, n_les, 8):
                s, tt = les.lesion_expand(*ops, bits, item, j0, min(8, n_les - j0))
                if crop:
                    s, tt = les._crop_pair(s, tt)
                boxes.append(list(s.shape))
                les._pair_counts(s, tt)
        chunks()
        cropped = [list(b) for b in boxes]
        t = alternate({'lesion_scores': lambda: mrdis.lesion_scores(labels, table), 'labelling': label_part,
                       'matching': lambda: les.lesion_match(*ops, n_les, words), 'per_lesion_scoring': chunks,
                       'lesion_scores_whole_volume': lambda: mrdis.lesion_scores(labels, table, crop=False),
                       'per_lesion_scoring_whole_volume': lambda: chunks(False),
                       'region_scores': lambda: mrdis.region_scores(labels, table)}, args.windows, args.iters)
        print(json.dumps({'metric': f'us per batch ({args.windows} alternating windows of {args.iters} calls); labelling = planes + dilation + two cc_label calls + '
                                    'running sums, per_lesion_scoring = expand + crop to the bounding box of the chunk + region_surfaces + surface_hist per chunk of 8 lesions; '
                                    '_whole_volume = the same with crop=False (the same bits)', 'config': cfg, 'lesions': n_les, 'chunks': (n_les + 7) // 8,
                          'cropped_chunk_shapes': cropped, **t,
                          'per_lesion_share': round(med(t['per_lesion_scoring']) / med(t['lesion_scores']), 2),
                          'beside': 'README: 90 ms per predict_volumes batch of this geometry, 7.5 ms per region_scores batch'}), flush=True)
    elif args.step == 'cpu':
        try:
            from scipy import ndimage
        except ImportError:
            print(json.dumps({'metric': 'scipy route', 'skipped': 'scipy is not importable here'}), flush=True)
            return
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = target[0].cpu().numpy()
        t1 = time.perf_counter()
        grown = ndimage.binary_dilation(host > 0, ndimage.generate_binary_structure(3, 2), iterations=3)
        t2 = time.perf_counter()
        lab, count = ndimage.label(grown, structure=np.ones((3, 3, 3), bool))
        t3 = time.perf_counter()
        ndimage.distance_transform_edt(~((lab == 1) & (host > 0)))
        t4 = time.perf_counter()
        print(json.dumps({'metric': 'ONE subject and ONE region through the CPU, ms: D2H copy of the ground truth, scipy binary_dilation (18-neighbourhood, 3 iterations), '
                                    'label (26-connected) of the dilated mask, and ONE distance_transform_edt of one lesion mask (a lesion takes two)',
                          'd2h_ms': round((t1 - t0) * 1e3, 2), 'dilation_ms': round((t2 - t1) * 1e3, 2), 'label_ms': round((t3 - t2) * 1e3, 2),
                          'edt_ms': round((t4 - t3) * 1e3, 2), 'lesions': int(count), 'per_batch': f'x {B} subjects x {R} regions; the transforms x 2 per lesion'}),
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join('profiles', 'lesion_bench.txt'))
    ap.add_argument('--windows', type=int, default=3)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--vol', type=int, nargs=3, default=[240, 240, 155])
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--step', choices=STEPS, help='run one step in this process (what the parent starts)')
    ap.add_argument('--step-timeout', type=int, default=150, help='time limit of every step, seconds')
    args = ap.parse_args()
    if args.step:
        return step(args)
    lines = [f'# Lesion-wise scoring (csrc/mrdis_lesion.hip) on one MI355X; tools/bench_lesion.py --windows {args.windows} --iters {args.iters}, one run, '
             'every step a process of its own.', '# See the tool\'s docstring for the scene, the bytes and store_only.']

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
