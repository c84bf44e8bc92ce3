"""Time the two kernels of the whole-subject 2-D segmentation (csrc/mrdis_seg2d.hip: hip.seg2d_label_planes, hip.seg2d_finish) on one MI355X
against a store-only pass over the same bytes and against the torch composition they replace, and one subject end to end -- all in ONE run.
    python tools/bench_seg2d.py [--out profiles/seg2d_bench.txt] [--windows 3] [--iters 20] [--no-subject]
Geometry: BraTS, 240 x 240 x 155, C = 4 classes, B = 32 centres per batch; n_sets (missing-contrast patterns) 1 and 15, views 1 and 2 (the second
W-flipped).  The subject end to end runs at the model's 160 x 192 crop (the network wants multiples of 32), M = 4, all 15 patterns.
Each figure: warm-up, then `windows` alternating windows of `iters` calls bracketed by device events; every window is printed (the spread).
Bytes are what the algorithm needs: label_planes = the logits of every set and view read + one byte per pixel and set written; finish = the
planes read + the (H, W, D) volumes written.  store_only = mrdis_stream_fill over a buffer of the same bytes.  torch = per set: flip the second
view back, softmax over the channels of both, mean, argmax (one view: argmax of the logits), 3 -> 4, cast to uint8, store into the planes
(label_planes); permute(0, 2, 3, 1).contiguous() (finish).
The subject's split: the same steps as segment_volumes, with a device synchronise between the phases (gather + anatomy encoders | fusion +
output decoders | the two new kernels | region scoring); the phases are timed in a run of their own, after the untimed-inside total."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mrdis  # noqa: E402

H, W, D, BLK, B, C = 240, 240, 155, 3, 32, 4
HS, WS = 160, 192                                   # the end-to-end subject: the model's input size
S0 = 67


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


def torch_labels(views, flips, planes, s0):
    dims = {1: 2, 2: 3}
    for s, vs in enumerate(views):
        if len(vs) == 1:
            lab = torch.argmax(vs[0], dim=1)
        else:
            ps = [torch.softmax(v.flip(dims[f]) if f else v, dim=1) for v, f in zip(vs, flips)]
            lab = torch.argmax(0.5 * (ps[0] + ps[1]), dim=1)
        lab = torch.where(lab == 3, torch.full_like(lab, 4), lab)
        planes[s, s0:s0 + vs[0].shape[0]] = lab.to(torch.uint8)


def med(v):
    return float(np.median(v))


def subject_split(model, cfg, store, names, pats):
    """one subject by the steps of segment_volumes -> ms per phase (a device synchronise after each phase)"""
    hip, seg = mrdis.hip, mrdis.segment
    Hs, Ws, Ds = store.shape
    dev = store.device
    ptrs = [store.ptr(f'S/{c}') for c in names]
    presents = [[c not in hid for c in names] for _, hid in pats]
    ms = {'encoders': 0.0, 'decoders': 0.0, 'seg2d_kernels': 0.0, 'scoring': 0.0}

    def lap(key, t0):
        torch.cuda.synchronize()
        ms[key] += (time.perf_counter() - t0) * 1e3
        return time.perf_counter()
    planes = torch.zeros((len(pats), Ds, Hs, Ws), dtype=torch.uint8, device=dev)
    model.eval()
    with torch.no_grad(), mrdis.ops.mix_cache():
        for s0, Bn in mrdis.synth_plan(Ds, BLK, B):
            t0 = time.perf_counter()
            idx = torch.arange(s0, s0 + Bn, dtype=torch.int32).to(dev)
            none = torch.full((Bn,), -1, dtype=torch.int32).to(dev)
            si = {}
            for vis in (True, False):
                row = torch.tensor([p if (i > 0 or vis) else 0 for i, p in enumerate(ptrs)], dtype=torch.int64).repeat(Bn, 1).to(dev)
                inputs, _, mask_img = hip.slice_gather(row, idx, none, Hs, Ws, Ds, BLK)
                si[vis] = seg.encode_anatomy(model, cfg, inputs, mask_img)
            t0 = lap('encoders', t0)
            views = []
            for pr in presents:
                mh = torch.tensor([[1.0 if p else 0.0 for p in pr]], dtype=torch.float32).repeat(Bn, 1)
                views.append([seg._dense_nhwc(model.output_decoder(mrdis.ops.fuse_present(si[pr[0]], mh.to(dev), mh, model.fuse_method))[0])])
            t0 = lap('decoders', t0)
            hip.seg2d_label_planes(views, [0], planes, s0, relabel=True)
            t0 = lap('seg2d_kernels', t0)
        t0 = time.perf_counter()
        labels = hip.seg2d_finish(planes)
        t0 = lap('seg2d_kernels', t0)
        target = store.vols['S/seg'].permute(1, 2, 0).contiguous()
        table = torch.full((len(pats),), target.data_ptr(), dtype=torch.int64).to(dev)
        mrdis.region_scores(labels, table)
        lap('scoring', t0)
    return {k: round(v, 1) for k, v in ms.items()}, labels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join('profiles', 'seg2d_bench.txt'))
    ap.add_argument('--windows', type=int, default=3)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--no-subject', action='store_true')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    hip = mrdis.hip
    torch.manual_seed(0)
    recs = []
    pool = [(3 * torch.randn(B, C, H, W, device=dev)).contiguous(memory_format=torch.channels_last) for _ in range(30)]
    for n_sets in (1, 15):
        for n_views in (1, 2):
            views = [[pool[s * n_views + v] for v in range(n_views)] for s in range(n_sets)]
            flips = [0, 2][:n_views]
            planes = torch.zeros((n_sets, D, H, W), dtype=torch.uint8, device=dev)
            planes_t = torch.zeros_like(planes)
            hip.seg2d_label_planes(views, flips, planes, S0, relabel=True)
            torch_labels(views, flips, planes_t, S0)
            differ = int((planes != planes_t).sum())
            nbytes = n_sets * n_views * B * C * H * W * 4 + n_sets * B * H * W
            fill_buf = torch.empty(nbytes // 16 * 4, device=dev)
            t = alternate({'kernel': lambda: hip.seg2d_label_planes(views, flips, planes, S0, relabel=True),
                           'torch': lambda: torch_labels(views, flips, planes_t, S0),
                           'store_only': lambda: hip.stream_fill(fill_buf)}, args.windows, args.iters)
            recs.append({'metric': f'mrdis_seg2d_label_planes, n_sets {n_sets}, views {n_views}, us per call ({args.windows} alternating windows)',
                         'config': f'B {B}, C {C}, {H} x {W}, D {D}', **t, 'moved_mb': round(nbytes / 1e6, 1),
                         'note': 'moved = logits read + label bytes written',
                         'tb_per_s': round(nbytes / med(t['kernel']) / 1e6, 2), 'store_only_tb_per_s': round(nbytes / med(t['store_only']) / 1e6, 2),
                         'kernel_over_store_only': round(med(t['kernel']) / med(t['store_only']), 2),
                         'torch_over_kernel': round(med(t['torch']) / med(t['kernel']), 2),
                         'voxels_differing_from_torch_one_call': differ, 'voxels': n_sets * B * H * W})
            print(json.dumps(recs[-1]), flush=True)
            del fill_buf, planes_t
            if n_views == 1:
                full = torch.randint(0, 5, (n_sets, D, H, W), dtype=torch.uint8, device=dev)
                out_k = hip.seg2d_finish(full)
                equal = bool(torch.equal(out_k, full.permute(0, 2, 3, 1).contiguous()))
                nb = 2 * n_sets * D * H * W
                fill_buf = torch.empty(nb // 16 * 4, device=dev)
                t = alternate({'kernel': lambda: hip.seg2d_finish(full), 'torch': lambda: full.permute(0, 2, 3, 1).contiguous(),
                               'store_only': lambda: hip.stream_fill(fill_buf)}, args.windows, args.iters)
                recs.append({'metric': f'mrdis_seg2d_finish, n_sets {n_sets}, us per call ({args.windows} alternating windows)',
                             'config': f'{D} x {H} x {W} uint8', **t, 'moved_mb': round(nb / 1e6, 1), 'note': 'moved = planes read + volumes written',
                             'tb_per_s': round(nb / med(t['kernel']) / 1e6, 2), 'store_only_tb_per_s': round(nb / med(t['store_only']) / 1e6, 2),
                             'kernel_over_store_only': round(med(t['kernel']) / med(t['store_only']), 2),
                             'torch_over_kernel': round(med(t['torch']) / med(t['kernel']), 2), 'bit_equal_torch': equal})
                print(json.dumps(recs[-1]), flush=True)
                del fill_buf, full, out_k
            del planes
    del pool
    torch.cuda.empty_cache()
    if not args.no_subject:
        names = ['T1', 'T1c', 'T2', 'T2_FLAIR']
        cfg = dict(mrdis.DEFAULT_CONFIG)
        cfg.update(contrast_list=names, input_height=HS, input_width=WS, batch_size=B, lambda_recon_y_fused=1.0, out_num_ch=4, dataset_name='BraTS')
        cfg = mrdis.derive_config(cfg, dev)
        torch.manual_seed(10); np.random.seed(10)
        model = mrdis.build_model(cfg)
        g = np.random.RandomState(1)
        arrays = {f'S/{c}': g.randn(HS, WS, D).astype(np.float32) for c in names}
        arrays['S/seg'] = g.randint(0, 5, (HS, WS, D)).astype(np.float32)
        store = mrdis.VolumeStore.from_arrays(arrays, dev)
        pats = mrdis.seg_patterns(names, 'all')
        ms = []
        for k in range(3):
            hip.launch_counts(reset=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = next(mrdis.segment_volumes(model, cfg, store, ['S'], pats))
            torch.cuda.synchronize()
            ms.append(round((time.perf_counter() - t0) * 1e3, 1))
        lc = hip.launch_counts()
        split, labels = subject_split(model, cfg, store, names, pats)
        split, labels = subject_split(model, cfg, store, names, pats)          # the second: warm
        recs.append({'metric': 'segment_volumes, one complete subject, all 15 patterns, one view, ms (first call warms up)',
                     'config': f'{HS} x {WS} x {D}, M 4, batch {B}: {len(mrdis.synth_plan(D, BLK, B))} batches, random weights', 'ms': ms,
                     'seg2dlabels_launches': lc['seg2dlabels'], 'seg2dfinish_launches': lc['seg2dfinish'],
                     'split_ms_with_a_synchronise_per_phase': split, 'split_equals_segment_volumes': bool(torch.equal(labels, res['labels']))})
        print(json.dumps(recs[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(f'# Whole-subject 2-D segmentation (csrc/mrdis_seg2d.hip) on {torch.cuda.get_device_name(dev)}, fp32; tools/bench_seg2d.py --windows '
                f'{args.windows} --iters {args.iters}, one process, one run.\n# See the tool\'s docstring for what the bytes, store_only and torch rows are.\n')
        for r in recs:
            f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
