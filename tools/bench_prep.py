"""Time the preprocessing kernels (csrc/mrdis_prep.hip: hip.prep_stats, hip.prep_write) on one MI355X against a store-only pass over the same
bytes and against the host composition they replace, and the host's gz decode of one file -- all in ONE run.
    python tools/bench_prep.py [--out profiles/prep_bench.txt] [--windows 3] [--iters 50]
Geometry: one BraTS volume, 240 x 240 x 155 in the file's order, crop ((40, 40), (24, 24)) -> 160 x 192 x 155; int16 and float32 input; both
store layouts.  Each device figure: warm-up, then `windows` alternating windows of `iters` calls bracketed by device events; every window is
printed (the spread).  Bytes are what the algorithm needs: prep_stats = the raw volume read twice (ssd needs n and sum); prep_write = the
cropped raw voxels read + the fp32 volume written.  store_only = mrdis_stream_fill over a buffer of the same bytes.  One volume is 18 MB
(int16) or 36 MB (float32): every read after the first upload comes from the Infinity Cache, not from HBM, and so does the store-only buffer.
host = the reference's statements in numpy float64 (get_fdata's cast, nan_to_num, crop, the three statistics passes, the normalisation) and
store.add (transposed copy, cast, upload) for one volume, wall clock, best of three.  gz = read_nifti of the same int16 volume as .nii.gz
(gzip level 6, as nibabel writes it), wall clock, best of three: the host decode that bounds a whole-dataset load."""
import argparse
import gzip
import json
import os
import struct
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mrdis  # noqa: E402

H, W, D = 240, 240, 155
CROP = ((40, 40), (24, 24))
HC, WC = 160, 192


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


def scan(dtype, seed=0):
    """an MR-like volume (H, W, D): smooth positive values inside an ellipsoid, 0 outside"""
    g = np.random.RandomState(seed)
    yy, xx, zz = np.meshgrid(np.arange(H), np.arange(W), np.arange(D), indexing='ij')
    inside = ((yy - H / 2) / (0.30 * H)) ** 2 + ((xx - W / 2) / (0.36 * W)) ** 2 + ((zz - D / 2) / (0.45 * D)) ** 2 <= 1
    v = (600 + 200 * np.sin(yy / 9.0) * np.cos(xx / 11.0) + g.randint(0, 60, (H, W, D))) * inside
    return v.astype(dtype)


def host_rule(img_file_order, store, key):
    """the reference's statements (data_preprocessing_BraTS.py:79-96) on the host, then store.add"""
    img = img_file_order.transpose(2, 1, 0).astype(np.float64)          # get_fdata
    img = np.nan_to_num(img, nan=0.)
    img = img[40:-40, 24:-24]
    brain_mask = (img > 0).astype(int)
    img_pos_num = (img > 0).sum()
    norm = img.sum() / (img_pos_num + 1)
    std = np.sqrt((brain_mask * (img - norm) ** 2).sum() / (img_pos_num + 1))
    img = (img - norm) / (std + 1e-8)
    img[brain_mask == 0] = -10
    store.add(key, img)
    return img


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join('profiles', 'prep_bench.txt'))
    ap.add_argument('--windows', type=int, default=3)
    ap.add_argument('--iters', type=int, default=50)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    hip = mrdis.hip
    recs = []
    for name in ('int16', 'float32'):
        a = scan(name)
        file_order = np.ascontiguousarray(a.transpose(2, 1, 0))
        raw = torch.from_numpy(file_order).to(dev)
        eb = raw.element_size()
        stats = hip.prep_stats(raw, CROP)
        nb = 2 * H * W * D * eb
        fill = torch.empty(nb // 16 * 4, device=dev)
        t = alternate({'kernel': lambda: hip.prep_stats(raw, CROP), 'store_only': lambda: hip.stream_fill(fill)}, args.windows, args.iters)
        recs.append({'metric': f'mrdis_prep_stats, {name}, us per call ({args.windows} alternating windows; four launches per call)',
                     'config': f'{H} x {W} x {D} file order, crop {CROP}', **t, 'moved_mb': round(nb / 1e6, 1), 'note': 'moved = the raw volume read twice',
                     'tb_per_s': round(nb / med(t['kernel']) / 1e6, 2), 'store_only_tb_per_s': round(nb / med(t['store_only']) / 1e6, 2),
                     'kernel_over_store_only': round(med(t['kernel']) / med(t['store_only']), 2)})
        print(json.dumps(recs[-1]), flush=True)
        del fill
        for layout in ('dhw', 'hwd'):
            out = hip.prep_write(raw, stats, 'zscore', CROP, layout)
            nb = HC * WC * D * (eb + 4)
            fill = torch.empty(nb // 16 * 4, device=dev)
            t = alternate({'kernel': lambda: hip.prep_write(raw, stats, 'zscore', CROP, layout, out=out), 'store_only': lambda: hip.stream_fill(fill)},
                          args.windows, args.iters)
            recs.append({'metric': f'mrdis_prep_write zscore, {name} -> {layout}, us per call ({args.windows} alternating windows)',
                         'config': f'{H} x {W} x {D} file order, crop {CROP} -> {HC} x {WC} x {D} fp32', **t, 'moved_mb': round(nb / 1e6, 1),
                         'note': 'moved = cropped raw voxels read + fp32 volume written',
                         'tb_per_s': round(nb / med(t['kernel']) / 1e6, 2), 'store_only_tb_per_s': round(nb / med(t['store_only']) / 1e6, 2),
                         'kernel_over_store_only': round(med(t['kernel']) / med(t['store_only']), 2)})
            print(json.dumps(recs[-1]), flush=True)
            del fill
        # the host composition for one volume, and how far the device volume is from it
        host_ms = []
        for _ in range(3):
            store = mrdis.VolumeStore(dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            want = host_rule(file_order, store, 'S/T1')
            torch.cuda.synchronize()
            host_ms.append(round((time.perf_counter() - t0) * 1e3, 1))
        dev_ms = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            vol, _ = mrdis.prep_volume(file_order, 'zscore', CROP, 'dhw', device=dev)
            torch.cuda.synchronize()
            dev_ms.append(round((time.perf_counter() - t0) * 1e3, 2))
        got = vol.cpu().numpy().transpose(1, 2, 0)
        w32 = want.astype(np.float32)
        beyond = int((np.abs(got.astype(np.float64) - w32.astype(np.float64)) > np.spacing(np.abs(w32)).astype(np.float64)).sum())
        recs.append({'metric': f'one volume, {name}: host composition (numpy float64 rule + store.add) against prep_volume from the same host array '
                               f'(upload + five launches + synchronise), ms wall clock, three repeats',
                     'host_ms': host_ms, 'prep_volume_ms': dev_ms, 'host_over_device': round(min(host_ms) / min(dev_ms), 1),
                     'voxels_beyond_1_ulp_of_host': beyond, 'voxels': int(got.size)})
        print(json.dumps(recs[-1]), flush=True)
    # the host's gz decode of one int16 file
    a = scan('int16')
    hdr = bytearray(352)
    struct.pack_into('<i', hdr, 0, 348)
    struct.pack_into('<8h', hdr, 40, 3, H, W, D, 1, 1, 1, 1)
    struct.pack_into('<2h', hdr, 70, 4, 16)
    struct.pack_into('<3f', hdr, 108, 352.0, 1.0, 0.0)
    hdr[344:348] = b'n+1\0'
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'S_t1.nii.gz')
        with gzip.open(path, 'wb', compresslevel=6) as f:
            f.write(bytes(hdr) + np.ascontiguousarray(a.transpose(2, 1, 0)).tobytes())
        size = os.path.getsize(path)
        gz_ms = []
        for _ in range(3):
            t0 = time.perf_counter()
            raw_np, _ = mrdis.read_nifti(path)
            gz_ms.append(round((time.perf_counter() - t0) * 1e3, 1))
    recs.append({'metric': 'read_nifti of one int16 .nii.gz (gzip level 6) on the host, ms wall clock, three repeats', 'gz_ms': gz_ms,
                 'file_mb': round(size / 1e6, 2), 'raw_mb': round(raw_np.nbytes / 1e6, 1),
                 'note': 'a synthetic scan; a fold of about 2,500 such files costs this per file on one core, whatever the device does'})
    print(json.dumps(recs[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(f'# Preprocessing of raw scans (csrc/mrdis_prep.hip) on {torch.cuda.get_device_name(dev)}; tools/bench_prep.py --windows {args.windows} '
                f'--iters {args.iters}, one process, one run.\n# See the tool\'s docstring for what the bytes, store_only, host and gz rows are.\n')
        for r in recs:
            f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
