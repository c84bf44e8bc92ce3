"""Time the two kernels of the fusion over the present contrasts (csrc/mrdis_fuse.hip: hip.fuse_present_fwd / _bwd) on one MI355X against a
store-only pass over the same bytes and against the torch composition they replace -- all in ONE run.
    python tools/bench_fuse.py [--out profiles/fuse_bench.txt] [--windows 3] [--iters 400]
Geometry: B 32, K 4 anatomy maps of C 4 channels, 240 x 240, fp32 channels-last; a drop-off mask (every fourth sample lacks one contrast), for the
three methods.
Each figure: warm-up, then `windows` alternating windows of `iters` calls bracketed by device events; every window is printed (the spread).
Bytes are what the algorithm needs: forward = the present maps read + the (B, F C, H, W) output written; backward = dout read + (max and
mean-max-min only) the present maps read again + all K gradients written.  store_only = mrdis_stream_fill over a buffer of the same bytes.
torch forward = stack, where(mask), sum / count, amax, amin (cat for mean-max-min); torch backward = its autograd (retain_graph, the gradient
accumulation into the leaves included; amax / amin split a tie's gradient evenly, the kernel gives it to the lowest present index: values differ
on ties by design, so only the forward is compared)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mrdis  # noqa: E402

B, K, C, H, W = 32, 4, 4, 240, 240
METHODS = ('mean', 'max', 'mean-max-min')


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


def torch_fuse(srcs, mask, method):
    s = torch.stack(srcs, 1)
    pres = (mask == 1)[:, :, None, None, None]
    mean = torch.where(pres, s, torch.zeros((), device=s.device)).sum(1) / pres.sum(1).float()
    if method == 'mean':
        return mean
    mx = torch.where(pres, s, torch.full((), float('-inf'), device=s.device)).amax(1)
    if method == 'max':
        return mx
    mn = torch.where(pres, s, torch.full((), float('inf'), device=s.device)).amin(1)
    return torch.cat([mean, mx, mn], 1)


def med(v):
    return float(np.median(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join('profiles', 'fuse_bench.txt'))
    ap.add_argument('--windows', type=int, default=3)
    ap.add_argument('--iters', type=int, default=400)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    hip = mrdis.hip
    torch.manual_seed(0)
    srcs = [torch.softmax(torch.randn(B, C, H, W, device=dev), 1).contiguous(memory_format=torch.channels_last) for _ in range(K)]
    mh = np.ones((B, K), dtype=np.float32)
    for b in range(0, B, 4):
        mh[b, (b // 4) % K] = 0
    mask = torch.from_numpy(mh).to(dev)
    n_present = int(mh.sum())
    map_bytes = C * H * W * 4
    cfgtxt = f'B {B}, K {K}, C {C}, {H} x {W}, {n_present} of {B * K} (sample, contrast) maps present'
    recs = []
    for method in METHODS:
        F = 3 if method == 'mean-max-min' else 1
        out = hip.fuse_present_fwd(srcs, mask, method)
        ref = torch_fuse(srcs, mask, method)
        diff = float((out - ref).abs().max())
        dout = torch.randn(B, F * C, H, W, device=dev).contiguous(memory_format=torch.channels_last)
        outs = [torch.empty_like(s) for s in srcs]
        leaves = [s.clone().requires_grad_() for s in srcs]
        tout = torch_fuse(leaves, mask, method)
        fwd_bytes = n_present * map_bytes + B * F * map_bytes
        bwd_bytes = B * F * map_bytes + (0 if method == 'mean' else n_present * map_bytes) + B * K * map_bytes
        fill_f, fill_b = torch.empty(fwd_bytes // 16 * 4, device=dev), torch.empty(bwd_bytes // 16 * 4, device=dev)
        t = alternate({'kernel_fwd': lambda: hip.fuse_present_fwd(srcs, mask, method, out=out),
                       'torch_fwd': lambda: torch_fuse(srcs, mask, method),
                       'store_only_fwd': lambda: hip.stream_fill(fill_f),
                       'kernel_bwd': lambda: hip.fuse_present_bwd(dout, srcs, mask, method, outs=outs),
                       'torch_bwd': lambda: torch.autograd.backward(tout, dout, retain_graph=True),
                       'store_only_bwd': lambda: hip.stream_fill(fill_b)}, args.windows, args.iters)
        recs.append({'metric': f'mrdis_fuse_present ({method}), us per call ({args.windows} alternating windows)', 'config': cfgtxt, **t,
                     'fwd_moved_mb': round(fwd_bytes / 1e6, 1), 'bwd_moved_mb': round(bwd_bytes / 1e6, 1),
                     'fwd_tb_per_s': round(fwd_bytes / med(t['kernel_fwd']) / 1e6, 2), 'bwd_tb_per_s': round(bwd_bytes / med(t['kernel_bwd']) / 1e6, 2),
                     'fwd_kernel_over_store_only': round(med(t['kernel_fwd']) / med(t['store_only_fwd']), 2),
                     'bwd_kernel_over_store_only': round(med(t['kernel_bwd']) / med(t['store_only_bwd']), 2),
                     'fwd_torch_over_kernel': round(med(t['torch_fwd']) / med(t['kernel_fwd']), 2),
                     'bwd_torch_over_kernel': round(med(t['torch_bwd']) / med(t['kernel_bwd']), 2),
                     'fwd_max_abs_diff_to_torch': diff})
        print(json.dumps(recs[-1]), flush=True)
        del out, ref, dout, outs, leaves, tout, fill_f, fill_b
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(f'# Fusion over the present contrasts (csrc/mrdis_fuse.hip) on one MI355X (the runtime\'s device name: {torch.cuda.get_device_name(dev)}), fp32; tools/bench_fuse.py --windows '
                f'{args.windows} --iters {args.iters}, one process, one run.\n# See the tool\'s docstring for what the bytes, store_only and torch rows are.\n')
        for r in recs:
            f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
