"""Time the nearest-neighbour modality-code search (hip.cosine_top1, csrc/mrdis_zsearch.hip) against its two roofs and against the
reference's formulation on the same GPU (model.py:3396-3415, per query: repeat the query N times, compute_cosine, argmax, read the index
on the host as its print does).  Gallery N x D fp32, Q queries, random labels over 100 subjects.
    python tools/bench_zsearch.py [--out FILE] [--bursts 7] [--iters 20]
Kernel: warm-up, then `bursts` bursts of `iters` launches bracketed by device events; the median burst per launch.
Roofs: gallery bytes N*D*4 at 8 TB/s, 2*Q*N*D FLOP at 157 TF (fp32 matrix peak); 'share' = the larger roof's time / measured time."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mrdis  # noqa: E402

HBM_BPS, MFMA_FLOPS = 8.0e12, 157.0e12


def burst_us(fn, iters, bursts):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    per = []
    for _ in range(bursts):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        per.append(a.elapsed_time(b) * 1e3 / iters)
    return statistics.median(per)


def compute_cosine(x, y):                  # model.py:3407-3415 as the reference writes it
    x_norm = torch.sqrt(torch.sum(torch.pow(x, 2), 1) + 1e-8)
    x_norm = torch.max(x_norm, 1e-8 * torch.ones_like(x_norm))
    y_norm = torch.sqrt(torch.sum(torch.pow(y, 2), 1) + 1e-8)
    y_norm = torch.max(y_norm, 1e-8 * torch.ones_like(y_norm))
    return torch.sum(x * y, 1) / (x_norm * y_norm)


def reference_batch(G, Qm):
    """main_missing.py:416-420 for one source contrast: one compute_nearest_neighbour_z_by_s per query row"""
    out = []
    for b in range(Qm.shape[0]):
        tile = Qm[b].unsqueeze(0).repeat(G.shape[0], 1)
        out.append(int(torch.argmax(compute_cosine(G, tile))))         # print(idx_sel): a host sync per query
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--bursts', type=int, default=7)
    ap.add_argument('--iters', type=int, default=20)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    lines = [f'# bench_zsearch on {torch.cuda.get_device_name(dev)}: median of {args.bursts} bursts x {args.iters} launches; '
             f'roofs {HBM_BPS / 1e12:.0f} TB/s, {MFMA_FLOPS / 1e12:.0f} TF fp32 MFMA',
             f'{"N":>7} {"D":>5} {"Q":>3} {"kernel_us":>10} {"MB":>8} {"GFLOP":>7} {"hbm_us":>7} {"mfma_us":>7} {"bound":>5} {"share":>6} '
             f'{"ref_us":>10} {"speedup":>8}']
    print(lines[0]); print(lines[1])
    for N in (11500, 115000):
        for D in (480, 1024):
            G = torch.randn(N, D, device=dev)
            glab = torch.randint(0, 100, (N,), dtype=torch.int32, device=dev)
            for Q in (32, 64):
                Qm = torch.randn(Q, D, device=dev)
                qlab = torch.randint(0, 100, (Q,), dtype=torch.int32, device=dev)
                t = burst_us(lambda: mrdis.hip.cosine_top1(G, glab, Qm, qlab), args.iters, args.bursts)
                nbytes, flop = N * D * 4, 2.0 * Q * N * D
                t_mem, t_mma = nbytes / HBM_BPS * 1e6, flop / MFMA_FLOPS * 1e6
                bound = 'hbm' if t_mem >= t_mma else 'mfma'
                share = max(t_mem, t_mma) / t
                Gref = G                                                    # the reference searches ALL rows but the query subject's: same passes
                tr = burst_us(lambda: reference_batch(Gref, Qm), 1, 3)
                ln = (f'{N:>7} {D:>5} {Q:>3} {t:>10.1f} {nbytes / 1e6:>8.1f} {flop / 1e9:>7.2f} {t_mem:>7.1f} {t_mma:>7.1f} {bound:>5} {share:>6.2f} '
                      f'{tr:>10.0f} {tr / t:>7.0f}x')
                print(ln, flush=True)
                lines.append(ln)
            del G
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
