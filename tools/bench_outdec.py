"""ms per training step with each output decoder (target_model_name 'U', 'U+SA', 'U+SA+CA', 'U+SSA+CA'; lambda_recon_y = 1, BraTS segmentation
loss) at B = 32, M = 4, 256x256 (eager TrainStep), against the shipped config without a decoder, and the new kernels of csrc/mrdis_outdec.hip
against the ATen composition of the same operation at the level-1 and level-4 shapes of that step.  Writes profiles/outdec_bench.txt.

    python tools/bench_outdec.py [--steps 5 --warmup 2 --out profiles/outdec_bench.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import mrdis  # noqa: E402

DEV = torch.device('cuda:0')
DECODERS = [None, 'U', 'U+SA', 'U+SA+CA', 'U+SSA+CA']


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


def step_ms(decoder, B, M, H, steps, warmup):
    cfg = dict(mrdis.DEFAULT_CONFIG)
    cfg.update(contrast_list=[f'm{i}' for i in range(M)], input_height=H, input_width=H, batch_size=B)
    if decoder is not None:
        cfg.update(lambda_recon_y=1.0, out_num_ch=4, target_model_name=decoder)
    cfg = mrdis.derive_config(cfg, DEV)
    torch.manual_seed(10); np.random.seed(10)
    model = mrdis.build_model(cfg).train()
    step = mrdis.TrainStep(model, cfg)
    x, mask, mask_img = mrdis.synthetic_batch(B, M, H, H, seed=3)
    tg = torch.randint(0, 4, (B, 1, H, H), generator=torch.Generator().manual_seed(13)).float().to(DEV) if decoder else None
    args = (x.to(DEV).contiguous(memory_format=torch.channels_last), mask.to(DEV), mask_img.to(DEV), mask)
    torch.manual_seed(11); np.random.seed(11)
    r = timed(lambda: step(*args, targets=tg), steps, warmup)
    del step, model
    torch.cuda.empty_cache()
    return r


def kernel_rows(B, H, steps, warmup):
    """level 1: x = down_1 (B, 64, H/2, H/2), gate up_2 (B, 256, H/4, H/4); level 4: x = down_4 (B, 512, H/16, H/16), gate down_5 (B, 512, H/32)"""
    hip = mrdis.hip
    g = torch.Generator(device=DEV).manual_seed(0)

    def cl(t):
        return t.contiguous(memory_format=torch.channels_last)
    rows = []
    for level, C, hx, Cg in ((1, 64, H // 2, 256), (4, 512, H // 16, 512)):
        Hd = 64
        x = cl(torch.randn(B, C, hx, hx, device=DEV, generator=g)).requires_grad_()
        s = cl(torch.randn(B, C, hx, hx, device=DEV, generator=g))
        dy = cl(torch.randn(B, C, hx, hx, device=DEV, generator=g))
        buf = cl(torch.empty(B, 2 * C, hx, hx, device=DEV))
        wd = (torch.randn(Hd, C, device=DEV, generator=g) / C ** 0.5).requires_grad_()
        bd = torch.zeros(Hd, device=DEV).requires_grad_()
        wu = (torch.randn(C, Hd, device=DEV, generator=g) / 8).requires_grad_()
        bu = torch.zeros(C, device=DEV).requires_grad_()
        gt = cl(torch.randn(B, Cg, hx // 2, hx // 2, device=DEV, generator=g)).requires_grad_()
        dgd = cl(torch.randn(B, Cg, hx // 2, hx // 2, device=DEV, generator=g))
        al = torch.sigmoid(torch.randn(B, 1, hx // 2, hx // 2, device=DEV, generator=g)).requires_grad_()
        mb = x.numel() * 4 / 2 ** 20

        def ch_aten():
            a = torch.sigmoid(F.linear(F.relu(F.linear(x.mean((2, 3)), wd, bd)), wu, bu))
            return (1 + a[:, :, None, None]) * x + s

        def ch_hip():
            return mrdis.ops.channel_attention_skip(x, s, wd, bd, wu, bu, into=(buf, 0))

        def sd_aten():
            return (gt - torch.flip(gt, dims=[2])).abs()

        def rg_aten():
            return (1 + F.interpolate(al, size=(hx, hx), mode='bilinear', align_corners=False)) * x

        def fb(f, grad_in, dout):
            return lambda: torch.autograd.grad(f(), grad_in, dout)
        cases = [('channel attention + skip sum', f'x {C}ch {hx}x{hx} ({mb:.0f} MB)', ch_hip, ch_aten, [x, wd, bd, wu, bu], dy),
                 ('symmetric difference', f'gate {Cg}ch {hx // 2}x{hx // 2}', lambda: mrdis.ops.symmetric_difference(gt), sd_aten, [gt], dgd),
                 ('residual gate', f'x {C}ch {hx}x{hx}', lambda: mrdis.ops.residual_gate(x, al), rg_aten, [x, al], dy)]
        for name, shape, fh, fa, ins, dout in cases:
            with torch.no_grad():
                fwd_h, fwd_a = timed(fh, steps, warmup)[0], timed(fa, steps, warmup)[0]
            fb_h, fb_a = timed(fb(fh, ins, dout), steps, warmup)[0], timed(fb(fa, ins, dout), steps, warmup)[0]
            rows.append((level, name, shape, fwd_h, fwd_a, fb_h, fb_a))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--modalities', type=int, default=4)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'outdec_bench.txt'))
    a = ap.parse_args()
    lines = [f'# tools/bench_outdec.py: B = {a.batch}, M = {a.modalities}, {a.size}x{a.size}, lambda_recon_y = 1 (BraTS segmentation loss, 4 output '
             f'channels), compute_dtype f32, eager TrainStep; median / min of {a.steps} timed steps after {a.warmup} warm-up steps '
             f'({torch.cuda.get_device_name(0)})', '', f'{"target_model_name":26s} {"ms/step median":>15s} {"min":>9s} {"vs no decoder":>14s}']
    base = None
    for dec in DECODERS:
        med, mn = step_ms(dec, a.batch, a.modalities, a.size, a.steps, a.warmup)
        base = med if base is None else base
        lines.append(f'{dec or "(none: shipped config)":26s} {med:15.2f} {mn:9.2f} {med - base:+13.2f}')
        print(lines[-1], flush=True)
    lines += ['', 'the kernels against the ATen composition of the same operation (ms, median of 50; fwd+bwd = forward then torch.autograd.grad)',
              f'{"level":>5s}  {"operation":30s} {"shape":28s} {"fwd hip":>8s} {"fwd aten":>9s} {"f+b hip":>8s} {"f+b aten":>9s}']
    for level, name, shape, fh, fa, bh, ba in kernel_rows(a.batch, a.size, 50, 5):
        lines.append(f'{level:5d}  {name:30s} {shape:28s} {fh:8.3f} {fa:9.3f} {bh:8.3f} {ba:9.3f}')
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('wrote', a.out)


if __name__ == '__main__':
    main()
