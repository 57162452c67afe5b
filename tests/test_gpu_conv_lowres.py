"""GPU parity of the low-resolution split-K 3x3 convolution (conv3x3_lowres_kernel, csrc/mos_conv_lowres.inc: row tiles of up to
256 pixels, the halo of a 64-channel chunk staged once, weights streamed, chunk ranges summed in order by the reduce kernel) at the
smallest shapes where it can still go wrong. Operand recipe and tolerance rule are those of
test_gpu_primitives.py::test_conv3x3_nhwc: a few ulps of the output dtype against the fp32 emulation, 1 ulp against the unsplit
kernel (another fp32 summation order of the same products).

The FORWARD call of every case takes the split form (asserted first through mos_conv3x3_nhwc_workspace_bytes > 0, without which
the other assertions say nothing about this kernel). The backward-data call contracts over Cout <= 128 here, below the split
rule's K depth, so it runs the same four checks on whichever unsplit form its shape takes."""
import math

import pytest
import torch

from tests.test_gpu_primitives import DTYPES, _check

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    import mixofshow.hip.ops as ops
    from mixofshow.hip import lib
    lib.load()
    return ops


@pytest.fixture(scope='module')
def emu():
    from oracle import emu_ops
    return emu_ops


def _four_checks(ops, emu, name, dtype, x, w_ohwi, bias, tb, res, ref=None):
    """emulation / unsplit kernel / two consecutive calls / dense read against the channel-slice read at offsets 0 and 128."""
    B, Cin, H, W = x.shape
    y = ops.conv3x3_nhwc(x, w_ohwi, bias, tb, res)
    assert y.shape == (B, w_ohwi.shape[0], H, W) and y.is_contiguous(memory_format=torch.channels_last)
    _check(f'{name} vs emulation', y, emu.conv3x3_nhwc(x, w_ohwi, bias, tb, res) if ref is None else ref, dtype)
    _check(f'{name} vs unsplit', y, ops.conv3x3_nhwc(x, w_ohwi, bias, tb, res, split_k=False), dtype, ulps=1.0)
    assert torch.equal(ops.conv3x3_nhwc(x, w_ohwi, bias, tb, res), y), f'{name}: two consecutive calls differ'
    for lo, wide in ((0, Cin + 320), (128, Cin + 192)):
        big = torch.zeros(B, wide, H, W, dtype=dtype, device='cuda').contiguous(memory_format=torch.channels_last)
        big.normal_(generator=torch.Generator(device='cuda').manual_seed(5))
        big[:, lo:lo + Cin] = x
        sl = big[:, lo:lo + Cin]
        assert ops.nhwc_pixel_stride(sl) == wide
        assert torch.equal(ops.conv3x3_nhwc(sl, w_ohwi, bias, tb, res), y), f'{name}: channels {lo}..{lo + Cin} of {wide} differ from the dense read'


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('B,Cin,Cout,H,W,extras', [
    (1, 256, 64, 8, 8, ''),          # one tile, one n-tile, minimum K depth for the split rule
    (3, 256, 128, 8, 8, 'tr'),       # a pixel tile with fewer images than it holds; per-image tbias inside one tile
    (5, 320, 64, 8, 8, 'tr'),        # two pixel tiles with the second ragged; 5 chunks in ranges of 3 and 2
    (1, 320, 72, 7, 5, 'tr'),        # odd map; Cout not a multiple of the tile
    (2, 256, 64, 16, 16, 'r'),       # one image per tile; the halo's zero border on all four sides
    (1, 256, 128, 16, 24, 't'),      # tiles of ten and six image rows; halo rows that belong to the same image above and below
    (2, 576, 64, 8, 12, ''),         # non-square map; 9 chunks
])
def test_conv3x3_lowres(ops, emu, dtype, B, Cin, Cout, H, W, extras):
    from mixofshow.hip import lib as _lib
    assert _lib.load().mos_conv3x3_nhwc_workspace_bytes(B, H, W, Cin, Cout) > 0, 'the forward shape does not take the split form'
    g = torch.Generator(device='cpu').manual_seed(21)
    x = torch.randn(B, Cin, H, W, generator=g).to('cuda', dtype).contiguous(memory_format=torch.channels_last)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin)).to('cuda', dtype)
    bias = (torch.randn(Cout, generator=g) * 0.1).cuda()
    tb = torch.randn(B, Cout, generator=g).to('cuda', dtype) if 't' in extras else None
    res = torch.randn(B, Cout, H, W, generator=g).to('cuda', dtype).contiguous(memory_format=torch.channels_last) \
        if 'r' in extras else None
    _four_checks(ops, emu, f'conv3x3 low-res [{B}x{Cin}->{Cout}x{H}x{W} {extras}]', dtype, x, w.permute(0, 2, 3, 1).contiguous(), bias, tb, res)
    if Cout % 64 != 0:
        return                                   # backward-data contracts over Cout: the kernel needs Cout % 64 == 0 there
    # backward-data: dx = conv(dy, flip(W)^T) == autograd of the fp32 convolution
    dy = torch.randn(B, Cout, H, W, generator=g).to('cuda', dtype).contiguous(memory_format=torch.channels_last)
    w_bwd = w.flip(2, 3).permute(1, 2, 3, 0).contiguous()
    xf = torch.zeros(B, Cin, H, W, device='cuda', requires_grad=True)
    (dx_ref, ) = torch.autograd.grad(torch.nn.functional.conv2d(xf, w.float(), None, padding=1), xf, dy.float())
    _four_checks(ops, emu, f'conv3x3 low-res backward-data [{B}x{Cout}->{Cin}x{H}x{W}]', dtype, dy, w_bwd, None, None, None, ref=dx_ref)
