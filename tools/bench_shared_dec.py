"""ms per training step with the fully shared input decoder (config.yaml `shared_inp_dec: True`, SPADENew) at the bench configuration
(B = 32, M = 4, 256x256, adversarial loss on), eager and graph-replayed, against the shipped config (split decoders) on the same box:
the configurations are built once and timed in alternating rounds after their warm-up, so clock and thermal drift hit all of them alike.
Also times the alternative decode that DESIGN.md 4.15 weighs: the second half (sp4 - sp6, out) as ONE grouped call per layer over the M
labels on the batch-concatenated maps (SPADENewNotShared.forward with the list of labels, the anatomy maps shared), which needs the M label blocks
of the sp4 input concatenated first.  Writes profiles/shared_dec_bench.txt.

    python tools/bench_shared_dec.py [--steps 10 --warmup 3 --rounds 3 --out profiles/shared_dec_bench.txt]
    python tools/bench_shared_dec.py --only shared --steps 3 --warmup 2 --out none      # (under rocprofv3 --kernel-trace --stats)
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


def grouped_tail_decode(model):
    """the alternative decode: sp1 - sp3 once per label at batch M B (as the default), then sp4 - sp6 and out as one grouped call per layer
    over the M labels, the M B anatomy maps shared by every label block (ops.conv2d_grouped share_x); the label blocks of the sp4 input are
    concatenated (one copy).  Replaces model._shared_dec_all for this instance."""
    ops = mrdis.ops
    dec = model.input_decoder_list[0]

    def shared_dec_all(si_list, zi_list):
        if not ops.grouped_applies():
            return None
        key = ('shdec_grouped', id(si_list[0]), id(zi_list[0]))

        def make():
            M, B = model.modality_num, si_list[0].shape[0]
            model.premix('dec')
            s_cat = torch.cat(list(si_list), 0)
            types = [model._type(j, M * B) for j in range(M)]
            z_cat = torch.cat([dec.head(s_cat, zi_list[j].repeat(M, 1), types[j]) for j in range(M)], 0)
            y = mrdis.SPADENewNotShared.forward(dec, s_cat, z_cat, types)
            outs = {}
            for j, blk in enumerate(ops.split_batch(y, M)):
                for i, part in enumerate(ops.split_batch(blk, M)):
                    outs[(i, j)] = part
            return (list(si_list), list(zi_list), outs)
        return ops.step_cache(key, make)[2]
    model._shared_dec_all = shared_dec_all


CONFIGS = [('shipped (split decoders), eager', dict(shared_inp_dec=False), False, False),
           ('shared_inp_dec, eager', dict(shared_inp_dec=True), False, False),
           ('shipped (split decoders), graph', dict(shared_inp_dec=False), True, False),
           ('shared_inp_dec, graph', dict(shared_inp_dec=True), True, False),
           ('shared_inp_dec, grouped-layer alt., eager', dict(shared_inp_dec=True), False, True)]


def build(opts, graph, alt, B, M, H):
    cfg = dict(mrdis.DEFAULT_CONFIG)
    cfg.update(contrast_list=[f'm{i}' for i in range(M)], input_height=H, input_width=H, batch_size=B, lambda_adv_s=1.0, **opts)
    cfg = mrdis.derive_config(cfg, DEV)
    torch.manual_seed(10); np.random.seed(10)
    model = mrdis.build_model(cfg).train()
    if alt:
        grouped_tail_decode(model)
    step = mrdis.TrainStep(model, cfg)
    if graph:
        step = mrdis.GraphedTrainStep(step)
    x, mask, mask_img = mrdis.synthetic_batch(B, M, H, H, seed=3)
    args = (x.to(DEV).contiguous(memory_format=torch.channels_last), mask.to(DEV), mask_img.to(DEV), mask)
    return lambda: step(*args)


def timed(fn, steps):
    times = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--modalities', type=int, default=4)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--only', default=None, help="'shared' or 'shipped': that configuration's eager step only (profiling runs)")
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'shared_dec_bench.txt'))
    a = ap.parse_args()
    configs = CONFIGS
    if a.only:
        configs = [c for c in CONFIGS if not c[2] and not c[3] and c[1]['shared_inp_dec'] == (a.only == 'shared')]
    fns = []
    for name, opts, graph, alt in configs:
        fn = build(opts, graph, alt, a.batch, a.modalities, a.size)
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        fns.append((name, fn))
        print('built + warmed', name, flush=True)
    times = {name: [] for name, _ in fns}
    for r in range(a.rounds):
        for name, fn in (fns if r % 2 == 0 else fns[::-1]):            # alternate the order round by round
            fn()                                                        # one untimed step after the switch
            torch.cuda.synchronize()
            times[name] += timed(fn, a.steps)
    lines = [f'# tools/bench_shared_dec.py: B = {a.batch}, M = {a.modalities}, {a.size}x{a.size}, lambda_adv_s = 1, compute_dtype f32; '
             f'{a.rounds} alternating rounds of {a.steps} timed steps per configuration after {a.warmup} warm-up steps '
             f'({torch.cuda.get_device_name(0)})', '', f'{"configuration":44s} {"ms/step median":>15s} {"min":>9s} {"vs shipped":>11s}']
    base = {}
    for name, _ in fns:
        med, mn = float(np.median(times[name])), float(np.min(times[name]))
        mode = name.split(', ')[-1]
        ref = base.setdefault(mode, med) if name.startswith('shipped') else base.get(mode)
        rel = f'{100 * (med / ref - 1):+10.1f}%' if ref else ''
        lines.append(f'{name:44s} {med:15.2f} {mn:9.2f} {rel:>11s}')
        print(lines[-1], flush=True)
    if a.out != 'none':
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
        print('wrote', a.out)


if __name__ == '__main__':
    main()
