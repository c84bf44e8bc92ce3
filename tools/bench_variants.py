"""ms per training step of the `others` variants (config.yaml:67-70) at the bench configuration (B = 32, M = 4, 256x256, adversarial loss on,
eager TrainStep), against the shipped config, and the modality encoder's two-source first layer (csrc/mrdis_encs.hip) against
concatenation + the library's convolution, forward and backward.  Writes profiles/variants_bench.txt.

    python tools/bench_variants.py [--steps 10 --warmup 3 --out profiles/variants_bench.txt]
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
VARIANTS = [('shipped', {'mod_enc_s': False, 'ana_dec_act': 'softmax', 'old': False, 'softmax_remove_mask': True}),
            ('mod_enc_s+softmax', {'mod_enc_s': True, 'ana_dec_act': 'softmax', 'old': False}),
            ('softmax', {'mod_enc_s': False, 'ana_dec_act': 'softmax', 'old': False}),
            ('softplus', {'mod_enc_s': False, 'ana_dec_act': 'softplus', 'old': False}),
            ('mod_enc_s+softplus', {'mod_enc_s': True, 'ana_dec_act': 'softplus', 'old': False}),
            ('mod_enc_s+softmax_remove_mask', {'mod_enc_s': True, 'ana_dec_act': 'softmax', 'old': False, 'softmax_remove_mask': True})]


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


def step_ms(others, B, M, H, steps, warmup, cut_second_pass=False):
    cfg = dict(mrdis.DEFAULT_CONFIG)
    cfg.update(contrast_list=[f'm{i}' for i in range(M)], input_height=H, input_width=H, batch_size=B, lambda_adv_s=1.0, others=others)
    cfg = mrdis.derive_config(cfg, DEV)
    torch.manual_seed(10); np.random.seed(10)
    model = mrdis.build_model(cfg).train()
    if cut_second_pass:
        # the second encoder pass's maps detached (calls 2, 4, ... of compute_anatomy_encoding): the step without the latent-z loss's
        # backward through s_new into the anatomy network -- what that path costs, on its own
        orig, calls = model.compute_anatomy_encoding, [0]

        def cut(inputs_list, mask_img, need_maps=True):
            out = orig(inputs_list, mask_img, need_maps=need_maps)
            calls[0] += 1
            return [s.detach() for s in out] if calls[0] % 2 == 0 else out
        model.compute_anatomy_encoding = cut
    step = mrdis.TrainStep(model, cfg)
    x, mask, mask_img = mrdis.synthetic_batch(B, M, H, H, seed=3)
    args = (x.to(DEV).contiguous(memory_format=torch.channels_last), mask.to(DEV), mask_img.to(DEV), mask)
    torch.manual_seed(11); np.random.seed(11)
    r = timed(lambda: step(*args), steps, warmup)
    del step, model
    torch.cuda.empty_cache()
    return r


def layer_ms(B, H, steps, warmup):
    """the first layer at bench scale (one modality-encoder call: B images, x 7 + s 4 -> 16, 3x3 stride 2, LeakyReLU)"""
    hip = mrdis.hip
    Cx, Cs, Co = 7, 4, 16
    g = torch.Generator(device=DEV).manual_seed(0)
    x = torch.randn(B, Cx, H, H, device=DEV, generator=g).contiguous(memory_format=torch.channels_last)
    s = torch.randn(B, Cs, H, H, device=DEV, generator=g).softmax(1).contiguous(memory_format=torch.channels_last)
    w_tck = torch.randn(9, Cx + Cs, Co, device=DEV, generator=g) * 0.1
    w_tkc = w_tck.permute(0, 2, 1).contiguous()
    bias = torch.zeros(Co, device=DEV)
    y = hip.conv2d_2src_fwd(x, s, w_tck, bias, 3, 3, 2, 1, True)
    dy = torch.randn(y.shape, device=DEV, generator=g).contiguous(memory_format=torch.channels_last)
    xs = torch.cat([x, s], 1).contiguous(memory_format=torch.channels_last)

    def cat_fwd():
        c = torch.cat([x, s], 1).contiguous(memory_format=torch.channels_last)
        return hip.conv2d_fwd(c, w_tck, bias, 3, 3, 2, 1, True)

    def cat_bwd():
        d = hip.conv2d_bwd_data(dy, w_tkc, (H, H), 3, 3, 2, 1)
        d[:, :Cx].contiguous(memory_format=torch.channels_last); d[:, Cx:].contiguous(memory_format=torch.channels_last)    # the split of the cat's adjoint
        hip.conv2d_bwd_weight(xs, dy, 3, 3, 2, 1, need_bias=True)

    def two_fwd():
        return hip.conv2d_2src_fwd(x, s, w_tck, bias, 3, 3, 2, 1, True)

    def two_bwd():
        hip.conv2d_2src_bwd_data(dy, w_tkc, Cx, Cs, (H, H), 3, 3, 2, 1)
        hip.conv2d_2src_bwd_weight(x, s, dy, 3, 3, 2, 1, need_bias=True)
    return {k: timed(f, steps, warmup) for k, f in (
        ('cat+conv fwd', cat_fwd), ('two-source fwd', two_fwd),
        ('cat+conv bwd (dx, ds, dW, db)', cat_bwd), ('two-source bwd (dx, ds, dW, db)', two_bwd),
        ('  conv data gradient (11 ch)', lambda: hip.conv2d_bwd_data(dy, w_tkc, (H, H), 3, 3, 2, 1)),
        ('  two-source data gradient', lambda: hip.conv2d_2src_bwd_data(dy, w_tkc, Cx, Cs, (H, H), 3, 3, 2, 1)),
        ('  two-source data gradient, ds only', lambda: hip.conv2d_2src_bwd_data(dy, w_tkc, Cx, Cs, (H, H), 3, 3, 2, 1, need_dx=False)),
        ('  conv weight gradient (11 ch)', lambda: hip.conv2d_bwd_weight(xs, dy, 3, 3, 2, 1, need_bias=True)),
        ('  two-source weight gradient', lambda: hip.conv2d_2src_bwd_weight(x, s, dy, 3, 3, 2, 1, need_bias=True)))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--modalities', type=int, default=4)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'variants_bench.txt'))
    a = ap.parse_args()
    lines = [f'# tools/bench_variants.py: B = {a.batch}, M = {a.modalities}, {a.size}x{a.size}, lambda_adv_s = 1, compute_dtype f32, eager TrainStep; '
             f'median / min of {a.steps} timed steps after {a.warmup} warm-up steps ({torch.cuda.get_device_name(0)})',
             '', f'{"variant (others)":34s} {"ms/step median":>15s} {"min":>9s} {"vs shipped":>11s}']
    base = None
    for name, others in VARIANTS:
        med, mn = step_ms(others, a.batch, a.modalities, a.size, a.steps, a.warmup)
        base = med if base is None else base
        lines.append(f'{name:34s} {med:15.2f} {mn:9.2f} {med - base:+10.2f}')
        print(lines[-1], flush=True)
    med, mn = step_ms(VARIANTS[1][1], a.batch, a.modalities, a.size, a.steps, a.warmup, cut_second_pass=True)
    lines.append(f'{"mod_enc_s+softmax, s_new detached":34s} {med:15.2f} {mn:9.2f} {med - base:+10.2f}   '
                 '(not a training configuration: isolates the backward through the second pass\'s maps)')
    print(lines[-1], flush=True)
    lines += ['', f'first layer of the modality encoder, one call: {a.batch} images, 7 + 4 -> 16, 3x3 stride 2, LeakyReLU (ms, median / min of 50)']
    for k, (med, mn) in layer_ms(a.batch, a.size, 50, 5).items():
        lines.append(f'{k:34s} {med:15.3f} {mn:9.3f}')
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('wrote', a.out)


if __name__ == '__main__':
    main()
