"""Time the two assembly kernels of the whole-subject synthesis (csrc/mrdis_synth.hip: hip.synth_accum, hip.synth_finish) on one MI355X against a
store-only pass over the same bytes and against the torch composition they replace, and one subject end to end -- all in ONE run.
    python tools/bench_synth.py [--out profiles/synth_bench.txt] [--windows 3] [--iters 20] [--no-subject]
Geometry: BraTS, 240 x 240 x 155, C = 7 (block_size 3), B = 32 centres per batch, 3 sources (M = 4); the subject end to end runs at the model's
160 x 192 crop of it (the network wants multiples of 32).
Each figure: warm-up, then `windows` alternating windows of `iters` calls bracketed by device events; every window is printed (the spread).
Bytes are what the algorithm needs: accumulation = the channels it reads (centre: one channel in seven of every fetched line is used, so the
lines it touches are 7 times these bytes) + the covered planes of acc read and written; finish = acc read, acc written, the (H, W, D) copy written.
store_only = mrdis_stream_fill over a buffer of the same bytes.  torch = index the channel of every source, stack, sum, index_add_ into acc
and cnt per channel (accumulation); where(cnt > 0, acc / cnt, fill), permute, contiguous (finish)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mrdis  # noqa: E402

H, W, D, BLK, B, NSRC = 240, 240, 155, 3, 32, 3
C = 2 * BLK + 1
HS, WS = 160, 192                                   # the end-to-end subject: the model's input size
S0 = 67                                             # a middle batch: every plane it predicts is inside the volume


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


def torch_accum(srcs, acc, cnt, s0, c_lo, c_hi):
    r = torch.arange(srcs[0].shape[0], device=acc.device)
    n = torch.full((srcs[0].shape[0],), len(srcs), dtype=torch.int32, device=acc.device)
    for c in range(c_lo, c_hi + 1):
        val = torch.stack([x[:, c] for x in srcs]).sum(0)
        idx = r + (s0 + c - BLK)
        acc.index_add_(0, idx, val)
        cnt.index_add_(0, idx, n)


def torch_finish(acc, cnt, fill):
    vol = torch.where((cnt > 0)[:, None, None], acc / cnt.clamp_min(1).float()[:, None, None], torch.full((), fill, device=acc.device))
    return vol, vol.permute(1, 2, 0).contiguous()


def med(v):
    return float(np.median(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join('profiles', 'synth_bench.txt'))
    ap.add_argument('--windows', type=int, default=3)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--no-subject', action='store_true')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    hip = mrdis.hip
    torch.manual_seed(0)
    srcs = [torch.randn(B, C, H, W, device=dev).contiguous(memory_format=torch.channels_last) for _ in range(NSRC)]
    centres = range(S0, S0 + B)
    cfgtxt = f'{H} x {W} x {D}, C {C}, B {B}, {NSRC} sources'
    recs = []
    for mode, (c_lo, c_hi) in (('centre', (BLK, BLK)), ('mean', (0, 2 * BLK))):
        acc = torch.zeros(D, H, W, device=dev)
        cnt = torch.zeros(D, dtype=torch.int32, device=dev)
        acc_t, cnt_t = torch.zeros_like(acc), torch.zeros_like(cnt)
        hip.synth_accum(srcs, centres, acc, cnt, c_lo, c_hi)
        torch_accum(srcs, acc_t, cnt_t, S0, c_lo, c_hi)
        diff = float((acc - acc_t).abs().max())
        same_cnt = bool(torch.equal(cnt, cnt_t))
        nch = c_hi - c_lo + 1
        nbytes = B * nch * H * W * 4 * NSRC + 2 * (B + nch - 1) * H * W * 4
        fill_buf = torch.empty(nbytes // 16 * 4, device=dev)
        t = alternate({'kernel': lambda: hip.synth_accum(srcs, centres, acc, cnt, c_lo, c_hi),
                       'torch': lambda: torch_accum(srcs, acc_t, cnt_t, S0, c_lo, c_hi),
                       'store_only': lambda: hip.stream_fill(fill_buf)}, args.windows, args.iters)
        recs.append({'metric': f'mrdis_synth_accum ({mode}), us per call ({args.windows} alternating windows)', 'config': cfgtxt, **t,
                     'moved_mb': round(nbytes / 1e6, 1), 'note': 'moved = channels read + covered acc planes read and written',
                     'tb_per_s': round(nbytes / med(t['kernel']) / 1e6, 2), 'store_only_tb_per_s': round(nbytes / med(t['store_only']) / 1e6, 2),
                     'kernel_over_store_only': round(med(t['kernel']) / med(t['store_only']), 2),
                     'torch_over_kernel': round(med(t['torch']) / med(t['kernel']), 2), 'max_abs_diff_to_torch_one_call': diff, 'counts_equal_torch': same_cnt})
        print(json.dumps(recs[-1]), flush=True)
        del acc_t, cnt_t, fill_buf
    # finish: the kernel divides in place, so every call gets acc back from a pristine copy first; that copy is timed alone and taken off
    acc0 = torch.randn(D, H, W, device=dev) * 8
    cnt0 = torch.randint(1, 22, (D,), dtype=torch.int32, device=dev)
    cnt0[:BLK] = 0
    acc = acc0.clone()
    vol_k, out_k = hip.synth_finish(acc0.clone(), cnt0, -10.0)
    vol_t, out_t = torch_finish(acc0, cnt0, -10.0)
    equal = bool(torch.equal(vol_k, vol_t) and torch.equal(out_k, out_t))
    nbytes = 3 * D * H * W * 4
    fill_buf = torch.empty(nbytes // 16 * 4, device=dev)
    t = alternate({'copy_plus_kernel': lambda: hip.synth_finish(acc.copy_(acc0), cnt0, -10.0), 'copy': lambda: acc.copy_(acc0),
                   'torch': lambda: torch_finish(acc0, cnt0, -10.0), 'store_only': lambda: hip.stream_fill(fill_buf)}, args.windows, args.iters)
    kern = [round(a - b, 1) for a, b in zip(t['copy_plus_kernel'], t['copy'])]
    recs.append({'metric': f'mrdis_synth_finish, us per call ({args.windows} alternating windows)', 'config': f'{D} x {H} x {W}', 'kernel': kern, **t,
                 'moved_mb': round(nbytes / 1e6, 1), 'note': 'moved = acc read + acc written in place + (H, W, D) copy written; kernel = copy_plus_kernel - copy',
                 'tb_per_s': round(nbytes / med(kern) / 1e6, 2), 'store_only_tb_per_s': round(nbytes / med(t['store_only']) / 1e6, 2),
                 'kernel_over_store_only': round(med(kern) / med(t['store_only']), 2), 'torch_over_kernel': round(med(t['torch']) / med(kern), 2),
                 'bit_equal_torch': equal})
    print(json.dumps(recs[-1]), flush=True)
    del srcs, acc, acc0, fill_buf, vol_k, out_k, vol_t, out_t
    torch.cuda.empty_cache()
    if not args.no_subject:
        names = ['T1', 'T1c', 'T2', 'T2_FLAIR']
        cfg = dict(mrdis.DEFAULT_CONFIG)
        cfg.update(contrast_list=names, input_height=HS, input_width=WS, batch_size=B)
        cfg = mrdis.derive_config(cfg, dev)
        torch.manual_seed(10); np.random.seed(10)
        model = mrdis.build_model(cfg)
        g = np.random.RandomState(1)
        store = mrdis.VolumeStore.from_arrays({f'S/{c}': g.randn(HS, WS, D).astype(np.float32) for c in names}, dev)
        for block in ('centre', 'mean'):
            ms = []
            for k in range(3):
                hip.launch_counts(reset=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = next(mrdis.synthesize_volumes(model, cfg, store, ['S'], block=block))
                torch.cuda.synchronize()
                ms.append(round((time.perf_counter() - t0) * 1e3, 1))
            lc = hip.launch_counts()
            recs.append({'metric': f'synthesize_volumes, one complete subject, block {block}, ms (first call warms up)',
                         'config': f'{HS} x {WS} x {D}, M 4, batch {B}: {len(mrdis.synth_plan(D, BLK, B))} batches, 4 targets x 3 sources, random weights',
                         'ms': ms, 'synthaccum_launches': lc['synthaccum'], 'synthfinish_launches': lc['synthfinish'],
                         'targets': res['targets']})
            print(json.dumps(recs[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(f'# Whole-subject synthesis (csrc/mrdis_synth.hip) on {torch.cuda.get_device_name(dev)}, fp32; tools/bench_synth.py --windows {args.windows} '
                f'--iters {args.iters}, one process, one run.\n# See the tool\'s docstring for what the bytes, store_only and torch rows are.\n')
        for r in recs:
            f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
