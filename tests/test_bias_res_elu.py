"""The one-pass epilogue behind the convs left on MIOpen
(csrc/updown.hip k_bias_res_elu) and the ResBlock module built on it
(fastconv.CfxMiopenResBlock)."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

gpu = pytest.mark.gpu
CL = torch.channels_last_3d


@gpu
@pytest.mark.parametrize('elu', [True, False], ids=['elu', 'noelu'])
@pytest.mark.parametrize('res', [True, False], ids=['res', 'nores'])
@pytest.mark.parametrize('K', [48, 64, 5])  # 5: the scalar path
def test_kernel_vs_torch(K, res, elu):
    from chunkflow_amd.fastconv import get_cfx
    torch.manual_seed(K)
    y = torch.randn(2, K, 2, 5, 7, device='cuda').contiguous(
        memory_format=CL)
    b = torch.randn(K, device='cuda')
    r = torch.randn_like(y).contiguous(memory_format=CL) if res else None
    want = y + b.view(1, -1, 1, 1, 1)
    if res:
        want = want + r
    if elu:
        want = F.elu(want)
    got = y.clone(memory_format=torch.preserve_format)
    assert got.is_contiguous(memory_format=CL)
    n, k, d, h, w = got.shape
    get_cfx(0).bias_res_elu(got.data_ptr(), b.data_ptr(),
                            r.data_ptr() if res else None, n * d * h * w,
                            k, do_elu=elu)
    torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-4)


class _ResBlock(nn.Module):
    """the RSUNet block (examples/nets/rsunet.py)"""

    def __init__(self, c):
        super().__init__()
        self.conv1 = nn.Conv3d(c, c, 3, padding=1, bias=True)
        self.conv2 = nn.Conv3d(c, c, 3, padding=1, bias=True)
        self.act = nn.ELU(inplace=True)

    def forward(self, x):
        y = self.act(self.conv1(x))
        y = self.conv2(y)
        return self.act(x + y)


@gpu
@torch.no_grad()
def test_block_module_vs_original_c48():
    from chunkflow_amd import fastconv as fc
    torch.manual_seed(1)
    block = _ResBlock(48).cuda().eval().to(memory_format=CL)
    assert fc._miopen_resblock_like(block)
    assert not fc._miopen_resblock_like(_ResBlock(28))  # the ring's width
    x = torch.randn(1, 48, 2, 8, 8, device='cuda').contiguous(
        memory_format=CL)
    want = block(x.clone(memory_format=torch.preserve_format))
    got = fc.CfxMiopenResBlock(block, 0).cuda()(x)
    torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-4)
    # surgery picks it up
    holder = nn.ModuleList([block])
    assert fc.maybe_accelerate(holder, 0) == 1
    assert isinstance(holder[0], fc.CfxMiopenResBlock)
