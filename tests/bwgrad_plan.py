"""The host planner of the bf16 weight-gradient family (csrc/mrdis_bf16.hip: plan_bwgrad, plan_bwgrad_s2, the selection in mrdis_run_bwgrad),
replayed in Python for a given CU count: which kernel and instantiation a call launches, with how many tiles and slabs, without a GPU.
tests/test_conv_check.py holds every bf16 weight-gradient row of tests/test_gpu_conv_paths.py to it at 256 CUs; on the GPU the launch counters
are the proof, this replay only says in advance what they will show and why."""

CUS = 256


def cdiv(a, b):
    return -(-a // b)


def _tile(H, W):
    tw = 32
    while tw > 1 and tw // 2 >= W:
        tw >>= 1
    th = 128 // tw
    while th > 1 and th // 2 >= H:
        th >>= 1
    return tw, th, 128 // (tw * th)


def plan(N, Ci, Co, H, W, k=3, stride=1, pad=1, dtype='bf16', opts=None, ld_ok=True, cus=CUS):
    """-> None where the family declines (the caller's fallback takes the call), else a dict: kernel ('bwgrad' | 'bwgrad2' | 'bwgrad3' |
    'bwgrad_s2'), inst (the template arguments as the row ids spell them), tiles, splits, TW, TH, NB, ws (workspace bytes the family needs)"""
    opts = opts or {}
    bf = dtype == 'bf16'
    if not ld_ok:
        return None
    wci, wco = (2 if Ci % 64 == 0 else 1), (2 if Co > 32 else 1)
    nCiB, nCoB = cdiv(Ci, 32 * wci), cdiv(Co, 32 * wco)
    if stride == 2:
        if not bf or opts.get('debug_now16') or pad != 1 or k not in (3, 4) or H % 2 or W % 2:
            return None
        if (Ci % 32 != 0 and Ci != 16) or Co % 8 != 0 or Co < 16:
            return None
        Hc, Wc = H // 2, W // 2
        if N * Hc * Wc < 2048:
            return None
        tw, th, nb = _tile(Hc, Wc)
        tiles = cdiv(Hc, th) * cdiv(Wc, tw) * cdiv(N, nb)
        # per class: the taps of one parity in each axis; the window spans (k == 4: 2 taps per axis in every class; k == 3: 2 or 1)
        for pr in (0, 1):
            for pq in (0, 1):
                nh = len([r for r in range(k) if (r - pad) & 1 == pr]); nw = len([s for s in range(k) if (s - pad) & 1 == pq])
                npix = nb * (th + nh - 1) * (tw + nw - 1)
                if npix * 4 * wci > (4 if wci == 2 else 2) * 512:
                    return None
        splits = max(1, min(cdiv(cus, 4 * nCiB * nCoB), tiles))
        half = Ci == 16
        return dict(kernel='bwgrad_s2', inst=f'<{wci},{wco},{"HALF" if half else "false"}>', tiles=tiles, splits=splits, TW=tw, TH=th, NB=nb,
                    ws=4 * splits * (k * k * Ci * Co + Co) + 256)
    if k * k > 9 or 2 * pad != k - 1:
        return None
    if (Ci % 32 != 0 and not (Ci == 16 and bf)) or Co % 8 != 0 or Co < 16:
        return None
    if Co <= 32 and Ci < 128 and not bf:
        return None
    if N * H * W < 4096:
        return None
    tw, th, nb = _tile(H, W)
    tinh, tinw = th + k - 1, tw + k - 1
    if tinh > 255 or tinw > 255 or nb > 255:
        return None
    tiles = cdiv(H, th) * cdiv(W, tw) * cdiv(N, nb)
    npix = nb * tinh * tinw
    if npix * 4 * wci > (4 if wci == 2 else 2) * 512:
        return None
    lds = max(2 * 32 * (wco * 128 + wci * npix), 8 * 16 * 64 * 4)
    splits = max(1, min(cdiv(cus, nCiB * nCoB), tiles))
    out = dict(tiles=tiles, splits=splits, TW=tw, TH=th, NB=nb, ws=4 * splits * (k * k * Ci * Co + Co) + 256)
    if bf and Ci % 32 == 0 and opts.get('wino_pipe', 1) and k == 3:
        stage3 = 2 * (wco * 128 * 32 + cdiv(wci * npix, 16) * 512)
        lds3 = max(3 * stage3 + 1024, 32768)
        if lds3 <= 160 * 1024 and wci * npix <= 512 and tiles >= 3 * splits and opts.get('debug_mode') != 3010:
            return dict(out, kernel='bwgrad3', inst=f'<{wci},{wco}>')
        if 2 * lds <= 150 * 1024 and tiles >= 2 * splits:
            return dict(out, kernel='bwgrad2', inst=f'<{wci},{wco}>')
    ts = '__bf16' if bf else 'float'
    return dict(out, kernel='bwgrad', inst=f'<1,{wco},__bf16,HALF>' if Ci == 16 else f'<{wci},{wco},{ts}>')


def reduce_phase(splits):
    """which part of bwgrad_reduce_kernel's slab loop a call with `splits` slabs exercises: wave w takes the slabs w, w + 16, ...; the four-way
    unrolled body runs while k + 48 < splits, the tail takes the rest"""
    if splits <= 16:
        return 'one slab per wave at most'
    if splits <= 48:
        return 'tail only, several slabs per wave'
    if splits >= 65:
        return 'unrolled body + tail'
    return 'unrolled body for some waves'
