"""Time the export kernel (csrc/mrdis_export.hip: hip.export_volume) on one MI355X against a store-only pass over the same bytes and against the
torch composition it replaces, and the host's gzip write of one file -- all in ONE run.
    python tools/bench_export.py [--out profiles/export_bench.txt] [--windows 3] [--iters 50]
Geometry: BraTS, store volumes 160 x 192 x 155 in the (H', W', D) layout, crop ((40, 40), (24, 24)) -> files of 240 x 240 x 155.  Cases: uint8 labels
with 1 and with 15 volumes per call (the patterns of phase segment), a float32 copy (units 'store') and un-z-score to int16 (units 'scan').  Each
device figure: warm-up, then `windows` alternating windows of `iters` calls bracketed by device events; every window is printed (the spread).
Bytes are what the algorithm needs: the store volume read + the file-order canvas written.  store_only = mrdis_stream_fill over a buffer of the
same bytes.  torch = F.pad (with the fill), permute, contiguous and, for a conversion, the inverse rule in float64, round, clamp, to: what a user
writes today; its result is compared with the kernel's.  One volume is 4.8 MB (uint8) to 36 MB of canvas: everything but the 15-volume case
lives in the Infinity Cache.
gz = write_nifti of one label volume (uint8; a sphere of labels, as a segmentation is mostly background) and of one float32 volume in store units
(a synthetic z-scored scan with a -10 background) as .nii.gz at gzip levels 1 and 6, wall clock, best of three, with the file sizes: the host
deflate that bounds a file's write."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mrdis  # noqa: E402

H, W, D = 240, 240, 155
CROP = ((40, 40), (24, 24))
HC, WC = 160, 192
INT_RANGE = {torch.uint8: (0, 255), torch.int16: (-32768, 32767)}


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


def med(v):
    return float(np.median(v))


def torch_export(src, kind, stats, fill, dtype):
    """the composition a user writes today, for (B, H', W', D) volumes -> (B, D, W, H)"""
    (h0, h1), (w0, w1) = CROP
    x = src
    if kind == 'unzscore':
        n1 = stats[:, 0] + 1.0
        norm, std = (stats[:, 1] / n1).view(-1, 1, 1, 1), (stats[:, 2] / n1).sqrt().view(-1, 1, 1, 1)
        x = torch.where(src == -10.0, torch.zeros((), dtype=torch.float64, device=src.device), src.double() * (std + 1e-8) + norm)
    x = F.pad(x, (0, 0, w0, w1, h0, h1), value=fill).permute(0, 3, 2, 1).contiguous()
    if dtype in INT_RANGE and x.dtype != dtype:
        x = x.nan_to_num(0.0).round().clamp(*INT_RANGE[dtype])
    return x.to(dtype)


def brain(seed=0):
    """(H', W', D) float32 in store units: a smooth z-scored scan inside an ellipsoid, -10 outside; and uint8 labels: nested spheres"""
    g = np.random.RandomState(seed)
    yy, xx, zz = np.meshgrid(np.arange(HC), np.arange(WC), np.arange(D), indexing='ij')
    r = ((yy - HC / 2) / (0.45 * HC)) ** 2 + ((xx - WC / 2) / (0.45 * WC)) ** 2 + ((zz - D / 2) / (0.45 * D)) ** 2
    z = np.where(r <= 1, np.sin(yy / 9.0) * np.cos(xx / 11.0) + 0.3 * g.randn(HC, WC, D), -10.0).astype(np.float32)
    t = ((yy - 70) / 30.0) ** 2 + ((xx - 110) / 25.0) ** 2 + ((zz - 80) / 20.0) ** 2
    lab = np.select([t <= 0.2, t <= 0.6, t <= 1.0], [4, 1, 2], 0).astype(np.uint8)
    return z, lab


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join('profiles', 'export_bench.txt'))
    ap.add_argument('--windows', type=int, default=3)
    ap.add_argument('--iters', type=int, default=50)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    hip = mrdis.hip
    z, lab = brain()
    stats1 = torch.tensor([[1.5e6, 9.0e8, 1.4e11, 3000.0, 0.0]], dtype=torch.float64, device=dev)
    recs = []
    cases = [('uint8 labels, 1 volume per call', lab, 1, 'copy', 0.0, torch.uint8), ('uint8 labels, 15 volumes per call', lab, 15, 'copy', 0.0, torch.uint8),
             ('float32 copy (units store), 1 volume', z, 1, 'copy', -10.0, torch.float32),
             ('un-z-score to int16 (units scan), 1 volume', z, 1, 'unzscore', 0.0, torch.int16)]
    for name, vol, B, kind, fill, dtype in cases:
        src = torch.from_numpy(vol).to(dev).unsqueeze(0).repeat(B, 1, 1, 1).contiguous()
        stats = stats1.expand(B, 5).contiguous() if kind != 'copy' else None
        out = torch.empty((B, D, W, H), dtype=dtype, device=dev)
        nb = B * (HC * WC * D * src.element_size() + H * W * D * out.element_size())
        probe = torch.empty(nb // 16 * 4, device=dev)
        same = bool(torch.equal(hip.export_volume(src, CROP, 'hwd', kind, stats, fill, dtype), torch_export(src, kind, stats, fill, dtype)))
        t = alternate({'kernel': lambda: hip.export_volume(src, CROP, 'hwd', kind, stats, fill, dtype, out=out),
                       'store_only': lambda: hip.stream_fill(probe), 'torch': lambda: torch_export(src, kind, stats, fill, dtype)}, args.windows, args.iters)
        recs.append({'metric': f'mrdis_export_volume, {name}, us per call ({args.windows} alternating windows; one launch per call)',
                     'config': f'{B} x {HC} x {WC} x {D} (H\', W\', D) {str(src.dtype)[6:]} -> {B} x {D} x {W} x {H} {str(dtype)[6:]}, crop {CROP}', **t,
                     'moved_mb': round(nb / 1e6, 1), 'note': 'moved = store volumes read + file-order canvases written',
                     'tb_per_s': round(nb / med(t['kernel']) / 1e6, 2), 'store_only_tb_per_s': round(nb / med(t['store_only']) / 1e6, 2),
                     'kernel_over_store_only': round(med(t['kernel']) / med(t['store_only']), 2),
                     'torch_over_kernel': round(med(t['torch']) / med(t['kernel']), 2), 'equal_to_torch': same})
        print(json.dumps(recs[-1]), flush=True)
        del probe, out, src
    # the host's gzip write of one file
    lab_file = np.ascontiguousarray(hip.export_volume(torch.from_numpy(lab).to(dev), CROP, 'hwd').cpu().numpy())
    z_file = np.ascontiguousarray(hip.export_volume(torch.from_numpy(z).to(dev), CROP, 'hwd', fill=-10.0, dtype=torch.float32).cpu().numpy())
    with tempfile.TemporaryDirectory() as tmp:
        for name, v in (('uint8 labels', lab_file), ('float32 store units', z_file)):
            for level in (1, 6):
                path = os.path.join(tmp, 'v.nii.gz')
                ms = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    mrdis.write_nifti(path, v, compresslevel=level)
                    ms.append(round((time.perf_counter() - t0) * 1e3, 1))
                recs.append({'metric': f'write_nifti of one {name} .nii.gz on the host, gzip level {level}, ms wall clock, three repeats', 'gz_ms': ms,
                             'file_mb': round(os.path.getsize(path) / 1e6, 3), 'raw_mb': round(v.nbytes / 1e6, 1)})
                print(json.dumps(recs[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(f'# Export of store volumes to NIfTI order (csrc/mrdis_export.hip) on {torch.cuda.get_device_name(dev)}; tools/bench_export.py '
                f'--windows {args.windows} --iters {args.iters}, one process, one run.\n# See the tool\'s docstring for what the bytes, store_only, torch '
                f'and gz rows are.\n')
        for r in recs:
            f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
