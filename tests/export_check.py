"""The rule of mrdis_export_volume (include/mrdis.h) restated in numpy float64: what tests/test_export_cpu.py checks on hand-written values and
tests/test_gpu_export.py holds the kernel to.  A plain module: nothing here touches the device or the package."""
import numpy as np

INT_RANGE = {np.dtype('u1'): (0.0, 255.0), np.dtype('i2'): (-32768.0, 32767.0)}


def convert(y, dtype):
    """float64 values -> the destination dtype: float32 by one rounding; int16 / uint8 by NaN -> 0, round to nearest with ties to even, clamp to
    the type's range (so +-inf saturate)"""
    y = np.asarray(y, dtype=np.float64)
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        with np.errstate(over='ignore'):
            return y.astype(np.float32)
    lo, hi = INT_RANGE[dtype]
    r = np.rint(np.where(np.isnan(y), 0.0, y))              # np.rint: ties to even
    return np.clip(r, lo, hi).astype(dtype)


def norm_std(stats):
    """(norm, std) of (B, 5) float64 statistics in the layout of mrdis_prep_stats: n, sum, ssd, vmax, nan_inner"""
    stats = np.asarray(stats, dtype=np.float64).reshape(-1, 5)
    return stats[:, 1] / (stats[:, 0] + 1.0), np.sqrt(stats[:, 2] / (stats[:, 0] + 1.0))


def values(src, crop, layout, kind='copy', stats=None, fill=0.0):
    """y in float64, (B, D, W, H) in file order on the full canvas, before the conversion.  src: (B, H', W', D) for layout 'hwd' or
    (B, D, H', W') for 'dhw', uint8 or float32; crop ((h0, h1), (w0, w1)); kind 'copy' | 'unzscore' | 'unmean'; stats (B, 5) float64"""
    (h0, h1), (w0, w1) = crop
    src = np.asarray(src)
    assert src.ndim == 4 and src.dtype in (np.uint8, np.float32)
    s = src.transpose(0, 3, 2, 1) if layout == 'hwd' else src.transpose(0, 1, 3, 2)          # (B, D, W', H')
    B, D, Wc, Hc = s.shape
    y = s.astype(np.float64)
    if kind != 'copy':
        assert src.dtype == np.float32
        norm, std = norm_std(stats)
        norm, std = np.broadcast_to(norm, (B,)).reshape(B, 1, 1, 1), np.broadcast_to(std, (B,)).reshape(B, 1, 1, 1)
        if kind == 'unzscore':
            with np.errstate(invalid='ignore', over='ignore'):
                y = np.where(s == np.float32(-10.0), 0.0, y * (std + 1e-8) + norm)       # numpy rounds the product, then the sum: no contraction
        else:
            assert kind == 'unmean'
            with np.errstate(invalid='ignore', over='ignore'):
                y = y * norm
    out = np.full((B, D, Wc + w0 + w1, Hc + h0 + h1), float(fill), dtype=np.float64)
    out[:, :, w0:w0 + Wc, h0:h0 + Hc] = y
    return out


def export(src, crop, layout, kind='copy', stats=None, fill=0.0, dtype=np.uint8):
    """-> (the converted (B, D, W, H) array, the float64 values behind it)"""
    y = values(src, crop, layout, kind, stats, fill)
    return convert(y, dtype), y


def tie_margin(y):
    """the smallest distance of a finite value's fractional part from 0.5: an integer destination is compared exactly only where this is >= 1e-6"""
    y = np.asarray(y, dtype=np.float64)
    y = y[np.isfinite(y)]
    return float(np.abs(np.abs(y - np.floor(y)) - 0.5).min()) if y.size else 1.0
