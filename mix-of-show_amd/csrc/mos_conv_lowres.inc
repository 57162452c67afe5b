// mos_conv_lowres.inc — third form of the 3x3 convolution, for the low-resolution levels that take split-K (stride 1, no upsampled
// read). Included by mos_conv.hip inside its anonymous namespace, after conv_ksplit and conv_splitk_reduce_kernel.
//
// The raster split-K form fetches every activation run nine times per n-tile and a weight tile once per 64-pixel m-tile: per K
// tile a wave issues 4 LDS-DMA pieces for 8 MFMAs, and the pieces, not the matrix pipe, set the pace. Here a workgroup owns up to
// 256 output pixels made of WHOLE IMAGE ROWS x 64 output channels x a range of channel chunks:
//   pixel tile : `nimg` whole images (8x8: four, 8x12: two) or `tr` rows of one image (16x16: all sixteen, 16x24: ten)
//   halo image : per image of the tile a block of (tr + 2) x hwp rows of 64 channels; halo row
//                hr = img * blk + hy * hwp + hx  <->  image pixel (b0 + img, y0 + hy - 1, hx - 1), zeros outside the image (the
//                buffer bounds check deposits them). hwp = W + 2, or W + 8 where W % 8 == 4, so that eight consecutive pixels of
//                the tile always sit on eight halo rows that differ modulo 8 (the chunk swizzle only looks at row & 7)
//   staging    : the halo of one chunk goes to LDS ONCE by LDS-DMA, chunk-swizzled like the other forms, double-buffered across
//                chunks; the nine taps are row offsets (ty * hwp + tx) into it -- no activation is fetched per tap
//   weights    : the ring of three [64][64] tiles with counted vmcnt waits; K order (chunk, tap); per (chunk, tap) a wave issues 2
//                weight pieces and runs 32 MFMAs (16 per piece; the raster form: 2). Every wave multiplies its 64 pixels by all
//                64 output channels: 8 ds_read_b128 per 16 MFMAs (0.5 per MFMA: half the LDS array's rate)
//   lanes      : MFMA column l15 of pixel fragment i is tile pixel wave * 64 + i * 16 + ((l15 + 12) & 15): the ds_read_b128 lane
//                groups pair l15 {4..11} and {0..3, 12..15}, which this rotation makes two runs of eight consecutive pixels
//   split-K    : workgroup z of a (pixel tile, n-tile) walks chunks [z * cpz, (z + 1) * cpz) and leaves its fp32 tile in partial[z];
//                conv_splitk_reduce_kernel sums in z order and applies the epilogue (deterministic)
//   XCD map    : as the raster split form -- the pixel tiles of one (n-tile, chunk range) are consecutive multiples of 8 apart in
//                the grid, i.e. on one XCD, whose L2 then fetches that weight slice once
// tools/sim_conv_halo.py (run_lowres) transcribes the index arithmetic below; tests/test_conv_lowres_model_cpu.py runs it.

constexpr int LR_BN = 64, LR_PIX = 256, LR_HRMAX = 448, LR_NPWMAX = LR_HRMAX / 32;

struct LowresPlan {
    int nimg, tr, tpi, hwp, blk, hr, npw, mt, ksplit, cpz;
};

// Geometry and K ranges of the low-resolution form for a shape, or false where the shape keeps the raster split-K form.
// One workgroup per CU (136 KiB of LDS): the ranges are chosen so that (pixel tiles x n-tiles x ranges) stays within the 256 CUs
// and every range holds at least two chunks (the halo double buffer needs a successor to hide, and the fp32 partials --
// ksplit x M x Cout x 4 bytes written and read back -- would pass the weights' own size at 8x8 beyond ~20 ranges).
inline bool conv_lowres_plan(int B, int H, int Wd, int Cin, int Cout, LowresPlan* p) {
#ifdef MOS_CONV_NO_LOWRES
    return false;
#endif
    int kt_per = 0;
    if (conv_ksplit(B * H * Wd, Cout, Cin, &kt_per) <= 1) return false;
    if (Wd > 64) return false;
    const int hwp = Wd + 2 + (Wd % 8 == 4 ? 6 : 0);
    int nimg = 1, tr = H;
    if (H * Wd <= LR_PIX) {
        nimg = LR_PIX / (H * Wd);
        if (nimg > LR_HRMAX / ((H + 2) * hwp)) nimg = LR_HRMAX / ((H + 2) * hwp);
        if (nimg > B) nimg = B;
    } else {
        tr = LR_PIX / Wd;
        while (tr > 0 && (tr + 2) * hwp > LR_HRMAX) --tr;
    }
    if (nimg < 1 || tr < 1) return false;
    p->nimg = nimg; p->tr = tr; p->hwp = hwp;
    p->tpi = (H + tr - 1) / tr;
    p->blk = (tr + 2) * hwp;
    p->hr = nimg * p->blk;
    p->npw = ((p->hr + 7) / 8 + 3) / 4;
    p->mt = ((B + nimg - 1) / nimg) * p->tpi;
    const int cpt = Cin / 64, units = p->mt * ((Cout + LR_BN - 1) / LR_BN);
    int ks = 256 / units;
    if (ks > cpt / 2) ks = cpt / 2;
    if (ks < 2) return false;
    p->cpz = (cpt + ks - 1) / ks;
    p->ksplit = (cpt + p->cpz - 1) / p->cpz;
    return p->ksplit >= 2;
}

// counted wait with a run-time (wave-uniform) count: s_waitcnt takes an immediate, so one case per count
__device__ __forceinline__ void wait_vmcnt_rt_then_barrier(int n) {
#define MOS_LR_CASE(N) case N: wait_vmcnt_then_barrier<N>(); break;
    switch (n) {
        MOS_LR_CASE(3) MOS_LR_CASE(4) MOS_LR_CASE(5) MOS_LR_CASE(6) MOS_LR_CASE(7) MOS_LR_CASE(8) MOS_LR_CASE(9) MOS_LR_CASE(10)
        MOS_LR_CASE(11) MOS_LR_CASE(12) MOS_LR_CASE(13) MOS_LR_CASE(14) MOS_LR_CASE(15) MOS_LR_CASE(16)
        default: wait_vmcnt_then_barrier<0>(); break;
    }
#undef MOS_LR_CASE
}

template <typename T>
__global__ __launch_bounds__(256) void conv3x3_lowres_kernel(const ConvArgs a) {
    typedef typename MT<T>::v8 v8;
    constexpr int BN = LR_BN, MI = 4, NJ = 4, WCH = 2;
    constexpr int HB = LR_HRMAX * CBK;             // elements per halo buffer
    static_assert(LR_NPWMAX + WCH <= 16 && HB * sizeof(T) < 65536, "wait cases / ds_read immediate offsets");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    T* Hs = reinterpret_cast<T*>(smem_raw);        // [2][LR_HRMAX rows][64], chunk-swizzled halo images
    T* Ws = Hs + 2 * HB;                           // [3][BN][64]

    const int w = blockIdx.x;
    const int r = w >> 3;
    const int m_tile = r % a.mt;
    const int u = (r / a.mt) * 8 + (w & 7);        // unit = (n-tile, chunk range); its mt workgroups share XCD w & 7
    if (u >= a.nt * a.ksplit) return;
    const int n_tile = u % a.nt, zsplit = u / a.nt;
    const int c0 = zsplit * a.kt_per, c1 = min(a.cpt, c0 + a.kt_per);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, lg = lane >> 4;
    const int N = a.Cout, C = a.Cin, LX = a.ldx, H = a.H, Wd = a.Wd, B = a.B;
    const int K = 9 * C;
    const int nimg = a.lr_nimg, tr = a.lr_tr, hwp = a.lr_hwp, npw = a.lr_npw, tpi = a.lr_tpi;
    const int blk = (tr + 2) * hwp, HR = nimg * blk, pb = tr * Wd;
    const int b0 = (m_tile / tpi) * nimg, y0 = (m_tile % tpi) * tr;
    const int n0 = n_tile * BN;

    const rsrc_t xsrc = make_rsrc(a.X, (uint32_t)((((int64_t)B * H * Wd - 1) * LX + C) * (int64_t)sizeof(T)));
    const rsrc_t wsrc = make_rsrc(a.W, (uint32_t)((((int64_t)N - 1) * K + K) * (int64_t)sizeof(T)));
    const rsrc_t xdead = make_rsrc(a.X, 0u), wdead = make_rsrc(a.W, 0u);
    constexpr int OOBL = (int)0x80000000u;         // past any descriptor: the DMA deposits zeros

    // halo DMA sources: piece (wave + 4 i) holds halo rows 8 * piece .. + 8, lane = (row, physical chunk)
    int hoff[LR_NPWMAX], woff[WCH];
#pragma unroll
    for (int i = 0; i < LR_NPWMAX; ++i) {
        const int hr = (wave + 4 * i) * 8 + lane / 8;
        const int img = hr / blk, rem = hr - img * blk;
        const int hy = rem / hwp, hx = rem - hy * hwp;
        const int bb = b0 + img, yy = y0 + hy - 1, xx = hx - 1;
        const int lc = (lane % 8) ^ (hr & 7);
        hoff[i] = (hr < HR && bb < B && yy >= 0 && yy < H && xx >= 0 && xx < Wd) ? (((bb * H + yy) * Wd + xx) * LX + lc * 8) * (int)sizeof(T) : OOBL;
    }
#pragma unroll
    for (int i = 0; i < WCH; ++i) {
        const int q = tid + 256 * i, row = q / 8;
        woff[i] = (int)((((int64_t)(n0 + row)) * K + (((q % 8) ^ (row & 7)) * 8)) * (int64_t)sizeof(T));
    }

    // this lane's pixels: fragment i, MFMA column l15 <-> tile pixel pt; mout = its row of the output (-1: not a pixel of the map)
    int mout[MI], hadr[9][MI][2];
#pragma unroll
    for (int i = 0; i < MI; ++i) {
        const int pt = wave * 64 + i * 16 + ((l15 + 12) & 15);
        const int img = pt / pb, prem = pt - img * pb;
        const int py = prem / Wd, px = prem - py * Wd;
        const bool ok = img < nimg && b0 + img < B && y0 + py < H;
        mout[i] = ok ? ((b0 + img) * H + y0 + py) * Wd + px : -1;
        const int hrow0 = ok ? img * blk + py * hwp + px : 0;      // halo row of tap (0, 0); pixels off the map read row 0 ..
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int hrow = hrow0 + (tap / 3) * hwp + tap % 3;
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) hadr[tap][i][kk] = hrow * CBK + (((kk * 4 + lg) ^ (hrow & 7)) * 8);
        }
    }

    f32x4 acc[NJ][MI];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int i = 0; i < MI; ++i) acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};

    auto issue_halo = [&](int cch, int hb) {       // chunk cch -> halo buffer hb (past the range: zeros, no traffic)
        const bool live = cch < c1;
        const rsrc_t src = live ? xsrc : xdead;
        const int cb = live ? cch * CBK * (int)sizeof(T) : 0;
#pragma unroll
        for (int i = 0; i < LR_NPWMAX; ++i)
            if (i < npw) dma16s(src, Hs + hb * HB + (wave + 4 * i) * 512, hoff[i], cb);
    };
    auto issue_w = [&](int cch, int tap, int buf) {
        const bool live = cch < c1;
        const rsrc_t src = live ? wsrc : wdead;
        const int kb = live ? (tap * C + cch * CBK) * (int)sizeof(T) : 0;
        T* ws = Ws + buf * BN * CBK + wave * 512;
#pragma unroll
        for (int i = 0; i < WCH; ++i) dma16s(src, ws + i * 2048, woff[i], kb);
    };
    const T* wfrag = Ws + l15 * CBK;               // weight fragment rows j * 16 + l15: the swizzle is that of l15
    const int wsw = l15 & 7;

    // one channel chunk: nine taps over halo buffer HBUF (a compile-time constant: the K loop below is unrolled by two)
    auto chunk = [&](const int cch, auto hbuf_c) {
        constexpr int HBUF = decltype(hbuf_c)::value;
        const T* hs = Hs + HBUF * HB;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            // this step's weight tile has landed once only the younger pieces are outstanding: one weight tile, plus -- at tap 1 --
            // the next chunk's halo, issued at tap 0 in front of it
            if (tap == 1) wait_vmcnt_rt_then_barrier(WCH + npw); else wait_vmcnt_then_barrier<WCH>();
            if (tap == 0) issue_halo(cch + 1, 1 - HBUF);
            {
                const int t2 = tap + 2;
                issue_w(t2 >= 9 ? cch + 1 : cch, t2 >= 9 ? t2 - 9 : t2, t2 % 3);
            }
            const T* ws = wfrag + (tap % 3) * BN * CBK;
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                v8 bfrag[MI], afrag[NJ];
#pragma unroll
                for (int i = 0; i < MI; ++i) bfrag[i] = as_v8<T>(ld16(hs + hadr[tap][i][kk]));
#pragma unroll
                for (int j = 0; j < NJ; ++j) afrag[j] = as_v8<T>(ld16(ws + j * 16 * CBK + ((kk * 4 + lg) ^ wsw) * 8));
#pragma unroll
                for (int j = 0; j < NJ; ++j)
#pragma unroll
                    for (int i = 0; i < MI; ++i) acc[j][i] = MT<T>::mfma16(afrag[j], bfrag[i], acc[j][i]);
            }
        }
    };

    issue_halo(c0, 0);
    issue_w(c0, 0, 0);
    issue_w(c0, 1, 1);
    for (int cch = c0; cch < c1; cch += 2) {
        chunk(cch, std::integral_constant<int, 0>{});
        if (cch + 1 < c1) chunk(cch + 1, std::integral_constant<int, 1>{});
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // the zero pieces issued past the range

    // raw fp32 partial tile; the reduce kernel owns the epilogue
    float* P = a.partial + (int64_t)zsplit * a.M * N;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int n = n0 + j * 16 + lg * 4;
#pragma unroll
        for (int i = 0; i < MI; ++i)
            if (mout[i] >= 0 && n < N) *reinterpret_cast<f32x4*>(P + (int64_t)mout[i] * N + n) = acc[j][i];   // N % 8 == 0
    }
}

template <typename T>
int launch_conv_lowres(ConvArgs a, const LowresPlan& p, hipStream_t st) {
    const size_t lds = ((size_t)2 * LR_HRMAX + (size_t)3 * LR_BN) * CBK * sizeof(T);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3x3_lowres_kernel<T>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    a.mt = p.mt;
    a.nt = (a.Cout + LR_BN - 1) / LR_BN;
    a.ksplit = p.ksplit; a.kt_per = p.cpz;        // kt_per: CHUNKS per range in this form
    a.lr_nimg = p.nimg; a.lr_tr = p.tr; a.lr_hwp = p.hwp; a.lr_npw = p.npw; a.lr_tpi = p.tpi;
    const int units8 = (a.nt * a.ksplit + 7) / 8;
    hipLaunchKernelGGL((conv3x3_lowres_kernel<T>), dim3(8 * units8 * a.mt), dim3(256), lds, st, a);
    int rc = mos_check_launch("conv3x3_nhwc(low-res split-K)");
    if (rc) return rc;
    const int64_t chunks = (int64_t)a.M * (a.Cout / 8);
    hipLaunchKernelGGL((conv_splitk_reduce_kernel<T>), dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, st, a);
    return mos_check_launch("conv_splitk_reduce");
}
