"""Lane-level model of the data movement of conv3x3_halo_kernel (csrc/mos_conv.hip; the default 3x3 path since round 5): LDS as an element array, dma16 = 16 B per lane at
(wave-uniform base) + lane * 16 from a global byte offset (zeros out of range), ld16 = 8 elements at an LDS element address, the
16x16x32 MFMA by its lane layout. The kernel's index arithmetic is transcribed literally; the sum is compared with conv2d.
The same model with the raster kernel's arithmetic (known to be right on the device) validates the model itself."""
import numpy as np
import torch

CBK = 64


def mfma16(acc, afrag, bfrag):
    """acc[lane][r] (D row = (lane >> 4) * 4 + r, col = lane & 15) += sum_k A[row][k] B[k][col];
    afrag[lane] = A[row = lane & 15][k = (lane >> 4) * 8 + e], bfrag[lane] = B[k = (lane >> 4) * 8 + e][col = lane & 15]."""
    A = np.zeros((16, 32)); Bm = np.zeros((32, 16))
    for lane in range(64):
        A[lane & 15, (lane >> 4) * 8:(lane >> 4) * 8 + 8] = afrag[lane]
        Bm[(lane >> 4) * 8:(lane >> 4) * 8 + 8, lane & 15] = bfrag[lane]
    D = A @ Bm
    for lane in range(64):
        for r in range(4):
            acc[lane][r] += D[(lane >> 4) * 4 + r, lane & 15]


def swz(CK, row):
    return (row & 7) if CK == 64 else ((row >> 1) & 3)


def run_halo(x, w, TH, BN, up=False, CK=64):
    """x (B, H, W, C) NHWC, w (Cout, 3, 3, C). Returns y (B, H, W, Cout) computed tile by tile like the kernel.
    up: x is (B, H/2, W/2, C) and is read through a nearest 2x upsample (template parameter UP of the kernel).
    CK: channels per chunk (template parameter CK: 64 -> rows of 8 chunks, 32 -> rows of 4 chunks, 16 rows per DMA piece)."""
    B, H, Wd, C = x.shape
    Hsrc, Wsrc = H, Wd
    if up:
        H, Wd = 2 * H, 2 * Wd
    N = w.shape[0]
    K = 9 * C
    MI, NJ, WCH = TH // 2, BN // 32, BN * CK // 2048
    RPP, CPR, KK = 512 // CK, CK // 8, CK // 32
    HW18 = 18
    HR = (TH + 2) * HW18
    NP = (HR + RPP - 1) // RPP
    NPW = (NP + 3) // 4
    HB = NPW * 4 * 512
    assert (MI * HW18) % 8 == 0 and WCH >= 1
    xg = x.reshape(-1).astype(np.float64)           # element-addressed global memory (offsets below are in BYTES, 2 per element)
    wg = w.reshape(-1).astype(np.float64)
    y = np.zeros((B, H, Wd, N))
    tx_n, ty_n = (Wd + 15) // 16, (H + TH - 1) // TH
    mt, nt = B * tx_n * ty_n, (N + BN - 1) // BN
    cpt = C // CK

    def gload(mem, lane_off, uni_off, limit_bytes):
        """buffer load of 16 B at lane_off (VGPR) + uni_off (scalar offset); out of range (either reading of the hardware rule:
        with or without the scalar part in the check) -> zeros. Asserts that both readings agree for every access issued."""
        a_ = lane_off >= limit_bytes                       # scalar offset not part of the check
        b_ = lane_off >= limit_bytes - uni_off             # ... or subtracted from the record count
        assert a_ == b_, (lane_off, uni_off, limit_bytes)
        if a_:
            return np.zeros(8)
        o = lane_off + uni_off
        assert 0 <= o and o + 16 <= limit_bytes
        return mem[o // 2: o // 2 + 8]

    for m_tile in range(mt):
        for n_tile in range(nt):
            b, tr = divmod(m_tile, tx_n * ty_n)
            y0, x0 = (tr // tx_n) * TH, (tr - (tr // tx_n) * tx_n) * 16
            n0 = n_tile * BN
            lds_h = np.zeros(2 * HB)
            lds_w = np.zeros(3 * BN * CK)
            acc = {(wave, j, i): [[0.0] * 4 for _ in range(64)] for wave in range(4) for j in range(NJ) for i in range(MI)}
            OOB = 0x80000000

            def hoff(wave, lane, i):
                hr = (wave + 4 * i) * RPP + lane // CPR
                hy, hx = divmod(hr, HW18)
                yy, xx = y0 + hy - 1, x0 + hx - 1
                lc = (lane % CPR) ^ swz(CK, hr)
                ok = hr < HR and 0 <= yy < H and 0 <= xx < Wd
                ys, xs = (yy >> 1, xx >> 1) if up else (yy, xx)
                return (((b * Hsrc + ys) * Wsrc + xs) * C + lc * 8) * 2 if ok else OOB

            def issue_halo(cch, hb):
                live = cch < cpt
                limit = xg.size * 2 if live else 0          # past the last chunk: the descriptor of zero records
                cb = cch * CK * 2 if live else 0
                for wave in range(4):
                    for i in range(NPW):
                        base = hb * HB + (wave + 4 * i) * 512
                        for lane in range(64):
                            lds_h[base + lane * 8: base + lane * 8 + 8] = gload(xg, hoff(wave, lane, i), cb, limit)

            def issue_w(cch, tap, buf):
                live = cch < cpt
                limit = ((N - 1) * K + K) * 2 if live else 0
                kb = (tap * C + cch * CK) * 2 if live else 0
                for wave in range(4):
                    for i in range(WCH):
                        base = buf * BN * CK + wave * 512 + i * 2048
                        for lane in range(64):
                            q = wave * 64 + lane + 256 * i
                            row = q // CPR
                            wo = ((n0 + row) * K + ((q % CPR) ^ swz(CK, row)) * 8) * 2
                            lds_w[base + lane * 8: base + lane * 8 + 8] = gload(wg, wo, kb, limit)

            issue_halo(0, 0)
            for cch in range(cpt):
                issue_halo(cch + 1, (cch + 1) & 1)         # (timing is not modelled: buffers are distinct, order is irrelevant here;
                hsb = (cch & 1) * HB                       #  the call past the last chunk exercises the zero-record descriptor)
                for tap in range(9):
                    issue_w(cch, tap, tap % 3)
                    if cch == cpt - 1 and tap == 8:
                        issue_w(cpt, 0, 0)                 # a weight tile past the end: zeros through the dead descriptor
                    for wave in range(4):
                        wm, wn = wave >> 1, wave & 1
                        for kk in range(KK):
                            bfr = {i: [None] * 64 for i in range(MI)}
                            afr = {j: [None] * 64 for j in range(NJ)}
                            for lane in range(64):
                                l15, lg = lane & 15, lane >> 4
                                for i in range(MI):
                                    cst = (i + tap // 3) * HW18 + tap % 3
                                    hpat = (wm * MI * HW18 + l15) * CK + (((kk * 4 + lg) ^ swz(CK, l15 + (cst & 7))) * 8)   # hpat[cst & 7][kk]
                                    a0 = hsb + hpat + cst * CK
                                    bfr[i][lane] = lds_h[a0:a0 + 8].copy()
                                wsw = swz(CK, l15)
                                for j in range(NJ):
                                    a0 = (tap % 3) * BN * CK + (wn * (BN // 2) + l15) * CK + j * 16 * CK + ((kk * 4 + lg) ^ wsw) * 8
                                    afr[j][lane] = lds_w[a0:a0 + 8].copy()
                            for j in range(NJ):
                                for i in range(MI):
                                    mfma16(acc[(wave, j, i)], afr[j], bfr[i])
            for wave in range(4):
                wm, wn = wave >> 1, wave & 1
                for j in range(NJ):
                    for i in range(MI):
                        for lane in range(64):
                            l15, lg = lane & 15, lane >> 4
                            nl = wn * (BN // 2) + j * 16 + lg * 4
                            ml = (wm * MI + i) * 16 + l15
                            yy, xx = y0 + (ml >> 4), x0 + (ml & 15)
                            for r in range(4):
                                if yy < H and xx < Wd and n0 + nl + r < N:
                                    y[b, yy, xx, n0 + nl + r] = acc[(wave, j, i)][lane][r]
    return y


# ---- conv3x3_lowres_kernel (csrc/mos_conv_lowres.inc): row tiles of up to 256 pixels, halo staged once per chunk, split-K ----
LR_BN, LR_PIX, LR_HRMAX, LR_NS = 64, 256, 448, 3
B128_GROUPS = [list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)), list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32)),
               list(range(32, 36)) + list(range(44, 48)) + list(range(52, 60)), list(range(36, 44)) + list(range(48, 52)) + list(range(60, 64))]


def conv_ksplit(M, Cout, Cin):
    """conv_ksplit of mos_conv.hip: (ranges, K tiles per range) of the raster split-K form; ranges 1 = not split."""
    nk = 9 * (Cin // 64)
    if nk < 36:
        return 1, 0
    tiles = ((M + 63) // 64) * ((Cout + 63) // 64)
    if tiles > 320:
        return 1, 0
    ks = min((640 + tiles - 1) // tiles, nk // 6)
    if ks < 2:
        return 1, 0
    per = (nk + ks - 1) // ks
    return (nk + per - 1) // per, per


def lowres_plan(B, H, Wd, Cin, Cout):
    """conv_lowres_plan: the geometry and the chunk ranges, or None where the shape keeps the raster split-K form."""
    if conv_ksplit(B * H * Wd, Cout, Cin)[0] <= 1 or Wd > 64:
        return None
    hwp = Wd + 2 + (6 if Wd % 8 == 4 else 0)
    nimg, tr = 1, H
    if H * Wd <= LR_PIX:
        nimg = min(LR_PIX // (H * Wd), LR_HRMAX // ((H + 2) * hwp), B)
    else:
        tr = LR_PIX // Wd
        while tr > 0 and (tr + 2) * hwp > LR_HRMAX:
            tr -= 1
    if nimg < 1 or tr < 1:
        return None
    p = dict(nimg=nimg, tr=tr, hwp=hwp, tpi=(H + tr - 1) // tr, blk=(tr + 2) * hwp)
    p['hr'] = nimg * p['blk']
    p['npw'] = ((p['hr'] + 7) // 8 + 3) // 4
    p['mt'] = ((B + nimg - 1) // nimg) * p['tpi']
    cpt, units = Cin // 64, p['mt'] * ((Cout + LR_BN - 1) // LR_BN)
    ks = min(256 // units, cpt // 2)
    if ks < 2:
        return None
    p['cpz'] = (cpt + ks - 1) // ks
    p['ksplit'] = (cpt + p['cpz'] - 1) // p['cpz']
    return p if p['ksplit'] >= 2 else None


def lowres_lane_pixel(p, H, Wd, B, m_tile, wave, i, l15):
    """(output row m or -1, halo row of tap (0, 0)) of MFMA column l15 of pixel fragment i."""
    b0, y0 = (m_tile // p['tpi']) * p['nimg'], (m_tile % p['tpi']) * p['tr']
    pb = p['tr'] * Wd
    pt = wave * 64 + i * 16 + ((l15 + 12) & 15)
    img, prem = divmod(pt, pb)
    py, px = divmod(prem, Wd)
    ok = img < p['nimg'] and b0 + img < B and y0 + py < H
    return (((b0 + img) * H + y0 + py) * Wd + px if ok else -1), (img * p['blk'] + py * p['hwp'] + px if ok else 0)


def lowres_bank_conflicts(p, H, Wd, B):
    """Worst number of distinct addresses on one 16-byte bank slot within a ds_read_b128 lane group, over every halo fragment read
    (tile, wave, fragment, tap, k-half) of the geometry whose lanes all hold pixels of the map; 1 = conflict-free."""
    worst = 1
    for m_tile in range(p['mt']):
        for wave in range(4):
            for i in range(4):
                px = [lowres_lane_pixel(p, H, Wd, B, m_tile, wave, i, l15) for l15 in range(16)]
                if any(m < 0 for m, _ in px):
                    continue
                for tap in range(9):
                    for kk in range(2):
                        for grp in B128_GROUPS:
                            slots = {}
                            for lane in grp:
                                l15, lg = lane & 15, lane >> 4
                                hrow = px[l15][1] + (tap // 3) * p['hwp'] + tap % 3
                                addr = (hrow * CBK + (((kk * 4 + lg) ^ (hrow & 7)) * 8)) * 2
                                slots.setdefault((addr // 16) % 16, set()).add(addr)
                            worst = max(worst, max(len(v) for v in slots.values()))
    return worst


def run_lowres(x, w, ldx_pad=0):
    """x (B, H, W, C) NHWC, w (Cout, 3, 3, C): y (B, H, W, Cout) as conv3x3_lowres_kernel + the ordered sum over the chunk ranges
    compute it. ldx_pad: extra channels per pixel in memory (the channel-slice read: ldx = C + ldx_pad). Every DMA is asserted in
    range or out of range under both readings of the bounds rule (gload), every destination inside its buffer."""
    B, H, Wd, C = x.shape
    N = w.shape[0]
    K = 9 * C
    p = lowres_plan(B, H, Wd, C, N)
    assert p is not None, 'the shape keeps the raster split-K form'
    nimg, tr, hwp, npw, tpi, blk, HR = p['nimg'], p['tr'], p['hwp'], p['npw'], p['tpi'], p['blk'], p['hr']
    LX = C + ldx_pad
    xm = np.full((B, H, Wd, LX), 1e6)                  # (the padding channels would wreck the sum if a DMA touched them)
    xm[..., :C] = x
    xg = xm.reshape(-1)[:(B * H * Wd - 1) * LX + C].astype(np.float64)
    wg = w.reshape(-1).astype(np.float64)
    xlimit, wlimit = ((B * H * Wd - 1) * LX + C) * 2, ((N - 1) * K + K) * 2
    HB = LR_HRMAX * CBK
    cpt, nt = C // CBK, (N + LR_BN - 1) // LR_BN
    OOBL = 0x80000000
    M = B * H * Wd
    partial = np.full((p['ksplit'], M, N), np.nan)     # no zero-fill: every element must be written

    def gload(mem, lane_off, uni_off, limit_bytes):
        a_ = lane_off >= limit_bytes
        b_ = lane_off >= limit_bytes - uni_off
        assert a_ == b_, (lane_off, uni_off, limit_bytes)
        if a_:
            return np.zeros(8)
        o = lane_off + uni_off
        assert 0 <= o and o + 16 <= limit_bytes
        return mem[o // 2: o // 2 + 8]

    for m_tile in range(p['mt']):
        b0, y0 = (m_tile // tpi) * nimg, (m_tile % tpi) * tr
        for n_tile in range(nt):
            n0 = n_tile * LR_BN
            for zsplit in range(p['ksplit']):
                c0 = zsplit * p['cpz']
                c1 = min(cpt, c0 + p['cpz'])
                lds_h = np.full(2 * HB, np.nan)
                lds_w = np.full(LR_NS * LR_BN * CBK, np.nan)

                def hoff(wave, lane, i):
                    hr = (wave + 4 * i) * 8 + lane // 8
                    img, rem = divmod(hr, blk)
                    hy, hx = divmod(rem, hwp)
                    bb, yy, xx = b0 + img, y0 + hy - 1, hx - 1
                    lc = (lane % 8) ^ (hr & 7)
                    ok = hr < HR and bb < B and 0 <= yy < H and 0 <= xx < Wd
                    return (((bb * H + yy) * Wd + xx) * LX + lc * 8) * 2 if ok else OOBL

                def issue_halo(cch, hb):
                    live = cch < c1
                    limit = xlimit if live else 0
                    cb = cch * CBK * 2 if live else 0
                    for wave in range(4):
                        for i in range(npw):
                            base = hb * HB + (wave + 4 * i) * 512
                            assert base + 512 <= (hb + 1) * HB
                            for lane in range(64):
                                lds_h[base + lane * 8: base + lane * 8 + 8] = gload(xg, hoff(wave, lane, i), cb, limit)

                def issue_w(cch, tap, buf):
                    live = cch < c1
                    limit = wlimit if live else 0
                    kb = (tap * C + cch * CBK) * 2 if live else 0
                    for wave in range(4):
                        for i in range(2):
                            base = buf * LR_BN * CBK + wave * 512 + i * 2048
                            for lane in range(64):
                                q = wave * 64 + lane + 256 * i
                                row = q // 8
                                wo = ((n0 + row) * K + ((q % 8) ^ (row & 7)) * 8) * 2
                                lds_w[base + lane * 8: base + lane * 8 + 8] = gload(wg, wo, kb, limit)

                acc = np.zeros((4, 4, 4, 64, 4))       # [wave][j][i][lane][r]
                px = [[[lowres_lane_pixel(p, H, Wd, B, m_tile, wave, i, l15) for l15 in range(16)] for i in range(4)] for wave in range(4)]
                issue_halo(c0, 0)
                for cch in range(c0, c1):
                    hbuf = (cch - c0) & 1
                    issue_halo(cch + 1, 1 - hbuf)
                    for tap in range(9):
                        wbuf = ((cch - c0) * 9 + tap) % LR_NS      # the ring: tile t in buffer t % NS
                        issue_w(cch, tap, wbuf)
                        for wave in range(4):
                            for kk in range(2):
                                bfr = np.zeros((4, 64, 8)); afr = np.zeros((4, 64, 8))
                                for lane in range(64):
                                    l15, lg = lane & 15, lane >> 4
                                    for i in range(4):
                                        hrow = px[wave][i][l15][1] + (tap // 3) * hwp + tap % 3
                                        a0 = hbuf * HB + hrow * CBK + (((kk * 4 + lg) ^ (hrow & 7)) * 8)
                                        assert a0 + 8 <= (hbuf + 1) * HB
                                        bfr[i, lane] = lds_h[a0:a0 + 8]
                                    for j in range(4):
                                        a0 = wbuf * LR_BN * CBK + l15 * CBK + j * 16 * CBK + ((kk * 4 + lg) ^ (l15 & 7)) * 8
                                        afr[j, lane] = lds_w[a0:a0 + 8]
                                for j in range(4):
                                    for i in range(4):
                                        if all(m < 0 for m, _ in px[wave][i]):
                                            continue           # (a fragment off the map: its reads were checked, its sum is dropped)
                                        a4 = [list(r_) for r_ in acc[wave, j, i]]
                                        mfma16(a4, np.nan_to_num(afr[j]), np.nan_to_num(bfr[i], nan=1e6))
                                        acc[wave, j, i] = a4
                    if cch == c1 - 1:
                        issue_w(c1, 0, (wbuf + 1) % LR_NS)  # a weight tile past the range: zeros through the dead descriptor
                for wave in range(4):
                    for j in range(4):
                        for i in range(4):
                            for lane in range(64):
                                l15, lg = lane & 15, lane >> 4
                                n = n0 + j * 16 + lg * 4
                                m = px[wave][i][l15][0]
                                if m >= 0 and n < N:
                                    assert np.isnan(partial[zsplit, m, n:n + 4]).all(), 'written twice'
                                    partial[zsplit, m, n:n + 4] = acc[wave, j, i, lane]
    assert not np.isnan(partial).any(), 'a partial element was never written'
    y = np.zeros((M, N))
    for z in range(p['ksplit']):
        y += partial[z]
    return y.reshape(B, H, Wd, N)


if __name__ == '__main__':
    g = torch.Generator().manual_seed(0)
    for (B, H, Wd, C, N, TH, BN, CK) in ((1, 8, 16, 64, 64, 8, 64, 64), (2, 10, 20, 128, 64, 8, 64, 64), (1, 17, 33, 64, 128, 16, 128, 64),
                                         (1, 9, 16, 64, 96, 8, 64, 64), (1, 8, 16, 64, 64, 8, 64, 32), (2, 10, 20, 64, 128, 8, 128, 32),
                                         (1, 9, 17, 96, 96, 8, 128, 32), (1, 9, 17, 64, 40, 8, 64, 32), (1, 18, 21, 64, 128, 16, 128, 32)):
        x = torch.randn(B, H, Wd, C, generator=g, dtype=torch.float64)
        w = torch.randn(N, 3, 3, C, generator=g, dtype=torch.float64)
        ref = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), padding=1).permute(0, 2, 3, 1)
        got = torch.from_numpy(run_halo(x.numpy(), w.numpy(), TH, BN, CK=CK))
        err = (got - ref).abs().max().item()
        print(f'B{B} {H}x{Wd} C{C} N{N} TH{TH} BN{BN} CK{CK}: max|d| = {err:.3e}')
        assert err < 1e-9
    for (B, H, Wd, C, N, TH, BN, CK) in ((1, 8, 8, 64, 64, 8, 64, 64), (2, 5, 12, 64, 64, 8, 64, 64), (1, 8, 16, 64, 128, 16, 128, 64),
                                         (1, 8, 8, 64, 128, 8, 128, 32), (2, 5, 12, 32, 64, 8, 64, 32), (1, 9, 10, 32, 128, 16, 128, 32)):
        x = torch.randn(B, H, Wd, C, generator=g, dtype=torch.float64)
        w = torch.randn(N, 3, 3, C, generator=g, dtype=torch.float64)
        xu = torch.nn.functional.interpolate(x.permute(0, 3, 1, 2), scale_factor=2.0, mode='nearest')
        ref = torch.nn.functional.conv2d(xu, w.permute(0, 3, 1, 2), padding=1).permute(0, 2, 3, 1)
        got = torch.from_numpy(run_halo(x.numpy(), w.numpy(), TH, BN, up=True, CK=CK))
        err = (got - ref).abs().max().item()
        print(f'upsampled read: B{B} {H}x{Wd} -> {2 * H}x{2 * Wd} C{C} N{N} TH{TH} BN{BN} CK{CK}: max|d| = {err:.3e}')
        assert err < 1e-9
