"""The lane-level model of conv3x3_lowres_kernel (tools/sim_conv_halo.py: run_lowres) on the CPU, at the geometries of
tests/test_gpu_conv_lowres.py with fewer channels: row tiles of whole images / of image rows, the per-image halo blocks, the lane
rotation, the chunk ranges of the split, the channel-slice read. The model asserts every LDS-DMA in range or out of range under both
readings of the bounds rule, every destination and fragment read inside its buffer, and every partial element written exactly once
(the workspace is not zero-filled); its sum is compared with conv2d. The bank model shows the halo fragment reads conflict-free at
the maps the UNet runs (8x8, 16x16, 16x24, 8x12)."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import sim_conv_halo  # noqa: E402


@pytest.mark.parametrize('B,C,N,H,W,pad', [
    (1, 256, 64, 8, 8, 0),        # one tile of one image, two chunk ranges of two chunks
    (3, 256, 64, 8, 8, 64),       # three images in a tile that holds four; channel-slice read
    (5, 320, 64, 8, 8, 0),        # two tiles, the second with one image; ranges of 3 and 2 chunks
    (1, 320, 72, 7, 5, 0),        # odd map, Cout past the 64-wide tile
    (2, 256, 64, 16, 16, 0),      # one image per tile
    (1, 256, 64, 16, 24, 128),    # ten rows + six rows of one image: halo rows from the same image above / below
    (2, 256, 64, 8, 12, 0),       # W % 8 == 4: halo rows 20 wide
])
def test_lowres_model_matches_conv2d(B, C, N, H, W, pad):
    g = torch.Generator().manual_seed(4)
    x = torch.randn(B, H, W, C, generator=g, dtype=torch.float64)
    w = torch.randn(N, 3, 3, C, generator=g, dtype=torch.float64)
    ref = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), padding=1).permute(0, 2, 3, 1)
    got = torch.from_numpy(sim_conv_halo.run_lowres(x.numpy(), w.numpy(), ldx_pad=pad))
    assert got.shape == ref.shape
    assert (got - ref).abs().max().item() < 1e-9


@pytest.mark.parametrize('B,H,W,C,N', [(4, 8, 8, 1280, 1280), (4, 16, 16, 1280, 1280), (4, 16, 16, 2560, 1280), (2, 16, 24, 1280, 1280),
                                       (2, 8, 12, 2560, 1280), (1, 8, 8, 256, 64), (2, 8, 12, 576, 64)])
def test_lowres_fragment_reads_are_conflict_free(B, H, W, C, N):
    p = sim_conv_halo.lowres_plan(B, H, W, C, N)
    assert p is not None and p['hr'] <= sim_conv_halo.LR_HRMAX and p['npw'] * 32 >= p['hr'] and p['npw'] <= 14
    assert sim_conv_halo.lowres_bank_conflicts(p, H, W, B) == 1


def test_lowres_plan_bounds():
    """Every shape the plan accepts fits the kernel's fixed LDS image and wait cases; the partials stay below 16 ranges."""
    for B in (1, 2, 3, 4, 5, 8):
        for H in range(1, 40):
            for W in range(1, 70):
                for C, N in ((256, 64), (1280, 1280), (2560, 1280), (320, 72)):
                    p = sim_conv_halo.lowres_plan(B, H, W, C, N)
                    if p is None:
                        continue
                    assert 1 <= p['npw'] <= 14 and p['hr'] <= sim_conv_halo.LR_HRMAX
                    assert p['nimg'] * p['tr'] * W <= 256 and 2 * p['hwp'] + 2 < sim_conv_halo.LR_HRMAX
                    assert 2 <= p['ksplit'] <= 16 and p['cpz'] >= 2 and p['ksplit'] * p['cpz'] >= C // 64 > (p['ksplit'] - 1) * p['cpz']
                    assert p['mt'] * ((N + 63) // 64) * p['ksplit'] <= 256


def test_model_transcribes_the_lowres_kernel_source():
    src = open(os.path.join(ROOT, 'mix-of-show_amd', 'csrc', 'mos_conv_lowres.inc')).read()
    for needle in ('const int hwp = Wd + 2 + (Wd % 8 == 4 ? 6 : 0);',
                   'const int hr = (wave + 4 * i) * 8 + lane / 8;',
                   'const int lc = (lane % 8) ^ (hr & 7);',
                   'const int bb = b0 + img, yy = y0 + hy - 1, xx = hx - 1;',
                   'const int pt = wave * 64 + i * 16 + ((l15 + 12) & 15);',
                   'const int hrow0 = ok ? img * blk + py * hwp + px : 0;',
                   'hadr[tap][i][kk] = hrow * CBK + (((kk * 4 + lg) ^ (hrow & 7)) * 8);',
                   'const int b0 = (m_tile / tpi) * nimg, y0 = (m_tile % tpi) * tr;',
                   'p->npw = ((p->hr + 7) / 8 + 3) / 4;'):
        assert needle in src, needle
