"""ms per training step of the latent-code options of the reference's loss block (lambda_kl, is_distri_z, s_compact_method 'mean') at the
bench configuration (B = 32, M = 4, 256x256, adversarial loss on, eager TrainStep), against the shipped config, and the new kernels
(csrc/mrdis_latent.hip) on their own.  Writes profiles/latent_options_bench.txt.

    python tools/bench_latent_options.py [--steps 10 --warmup 3 --out profiles/latent_options_bench.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import mrdis  # noqa: E402

DEV = torch.device('cuda:0')
OPTIONS = [('shipped', {}),
           ('lambda_kl 1 (standard KL)', dict(lambda_kl=1.0)),
           ('is_distri_z + lambda_kl 1', dict(is_distri_z=True, lambda_kl=1.0)),
           ("s_compact_method 'mean'", dict(s_compact_method='mean')),
           ('all three', dict(is_distri_z=True, lambda_kl=1.0, s_compact_method='mean'))]


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), float(np.min(times))


def step_ms(opts, B, M, H, steps, warmup):
    cfg = dict(mrdis.DEFAULT_CONFIG)
    cfg.update(contrast_list=[f'm{i}' for i in range(M)], input_height=H, input_width=H, batch_size=B, lambda_adv_s=1.0, **opts)
    cfg = mrdis.derive_config(cfg, DEV)
    torch.manual_seed(10); np.random.seed(10)
    model = mrdis.build_model(cfg).train()
    step = mrdis.TrainStep(model, cfg)
    x, mask, mask_img = mrdis.synthetic_batch(B, M, H, H, seed=3)
    args = (x.to(DEV).contiguous(memory_format=torch.channels_last), mask.to(DEV), mask_img.to(DEV), mask)
    torch.manual_seed(11); np.random.seed(11)
    r = timed(lambda: step(*args), steps, warmup)
    del step, model
    torch.cuda.empty_cache()
    return r


def kernel_ms(B, M, H, steps, warmup):
    hip = mrdis.hip
    g = torch.Generator(device=DEV).manual_seed(0)
    mus = [torch.randn(B, 16, device=DEV, generator=g) for _ in range(M)]
    lvs = [0.3 * torch.randn(B, 16, device=DEV, generator=g) for _ in range(M)]
    w = torch.full((M, B), 1.0 / (M * B), device=DEV)
    pm, plv = torch.randn(M, 16, device=DEV, generator=g), torch.randn(M, 16, device=DEV, generator=g)
    one = torch.ones((), device=DEV)
    s = torch.randn(B, 4, H, H, device=DEV, generator=g).softmax(1).contiguous(memory_format=torch.channels_last)
    dy = torch.randn(B, 4 * (H // 16) ** 2, device=DEV, generator=g)
    dyc = dy.view(B, 4, H // 16, H // 16).contiguous(memory_format=torch.channels_last)
    y, arg = hip.maxpool_fwd(s, 16)
    return {k: timed(f, steps, warmup) for k, f in (
        ('kl forward, two-Gaussian', lambda: hip.kl_fwd(mus, lvs, w, pm, plv)),
        ('kl backward, two-Gaussian', lambda: hip.kl_bwd(one, mus, lvs, w, pm, plv)),
        ('mean compaction forward (one map)', lambda: hip.avgpool_fwd(s, 16)),
        ('max compaction forward (one map)', lambda: hip.maxpool_fwd(s, 16)),
        ('mean compaction backward', lambda: hip.avgpool_bwd(dy, tuple(s.shape), 16)),
        ('max compaction backward', lambda: hip.maxpool_bwd(dyc, arg, tuple(s.shape), 16)))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--modalities', type=int, default=4)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'latent_options_bench.txt'))
    a = ap.parse_args()
    lines = [f'# tools/bench_latent_options.py: B = {a.batch}, M = {a.modalities}, {a.size}x{a.size}, lambda_adv_s = 1, compute_dtype f32, eager '
             f'TrainStep; median / min of {a.steps} timed steps after {a.warmup} warm-up steps ({torch.cuda.get_device_name(0)})',
             '', f'{"option":34s} {"ms/step median":>15s} {"min":>9s} {"vs shipped":>11s}']
    base = None
    for name, opts in OPTIONS:
        med, mn = step_ms(opts, a.batch, a.modalities, a.size, a.steps, a.warmup)
        base = med if base is None else base
        lines.append(f'{name:34s} {med:15.2f} {mn:9.2f} {med - base:+10.2f}')
        print(lines[-1], flush=True)
    lines += ['', 'the kernels on their own, bench scale (ms, median / min of 50)']
    for k, (med, mn) in kernel_ms(a.batch, a.modalities, a.size, 50, 5).items():
        lines.append(f'{k:34s} {med:15.3f} {mn:9.3f}')
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('wrote', a.out)


if __name__ == '__main__':
    main()
