"""``cabi_x.mx_pack`` / ``mx_unpack`` on the GPU (include/fewbit_hipx.h, "The row blocks of a seed"; fewbit_amd/csrc/fewbit_mx.hip) BIT FOR BIT against the
host evaluation of the same definition (``mx_pack_host`` / ``mx_unpack_host``): every dtype and format at row counts around a block and widths around
a tile, a leading dimension that keeps the 16-byte loads and a source off its 16-byte alignment that does not, one column of tiny cells (amax about
2^-126: denormal elements and denormal decodes), guard bytes behind every output, one poisoned cell."""
import pytest
import torch

from fewbit_amd import cabi_x

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DTYPES = (torch.bfloat16, torch.float16, torch.float32)
ids = lambda v: str(v).split('.')[-1] if isinstance(v, torch.dtype) else None


def defined(packed, rows, width):
    """the bytes the definition covers: the scales and the codes, without the gap in front of the codes that the kernel leaves alone"""
    scales = -(-rows // 32) * width
    return torch.cat((packed[:scales], packed[-(-scales // 16) * 16:]))


@pytest.mark.parametrize('format', cabi_x.MX_FORMATS)
@pytest.mark.parametrize('dtype', DTYPES, ids=ids)
@pytest.mark.parametrize('layout', ('dense', 'ld', 'offset'))
def test_pack_and_unpack_are_the_host_forms_bytes(layout, dtype, format):
    for rows in (1, 31, 32, 33, 69):
        for width in (1, 33, 64 + 5, 72):                                   # (72 dense, and every width under `ld`: the 16-byte loads)
            gen = torch.Generator().manual_seed(rows * 100 + width)
            values = torch.randn(rows, width, generator=gen) * torch.logspace(-6, 6, width, base=2.0)
            values[:, -1] *= 2.0**-133                                        # (fp16 has no such values: a column of zero cells there)
            values = values.to(dtype)
            values[rows // 2, width // 3] = 0.0
            if rows == 33 and width == 33:
                values[32, 7] = float('inf')                                  # one poisoned cell: the one row of the last block
            ld = width if layout == 'dense' else -(-width // 8) * 8 + 8 if layout == 'ld' else width + 3
            off = 1 if layout == 'offset' else 0                              # `offset`: src one element off its 16-byte alignment, rows not 16 bytes apart
            store = torch.full((rows * ld + 1, ), float('nan'), dtype=dtype, device=DEV)
            src = store[off:off + rows * ld].view(rows, ld)[:, :width]
            src.copy_(values)
            need = cabi_x.mx_bytes(rows, width, format)
            whole = torch.full((need + 32, ), 0xA5, dtype=torch.uint8, device=DEV)
            packed = cabi_x.mx_pack(src, 2026 + rows, format, 'grad' if width == 33 else 'kept', out=whole[:need])
            again = cabi_x.mx_pack(src, 2026 + rows, format, 'grad' if width == 33 else 'kept')
            want = cabi_x.mx_pack_host(values.float(), 2026 + rows, format, 'grad' if width == 33 else 'kept')
            assert torch.equal(defined(packed.cpu(), rows, width), defined(want, rows, width)), (rows, width)
            assert torch.equal(defined(again, rows, width), defined(packed, rows, width)) and bool((whole[need:] == 0xA5).all())
            # the decode, into every dtype, behind the same kind of guard
            wanted = cabi_x.mx_unpack_host(want, rows, width, format)
            guard = torch.full((rows * width + 16, ), -7.0, dtype=dtype, device=DEV)
            got = cabi_x.mx_unpack(packed, rows, width, format, dtype, out=guard[:rows * width].view(rows, width))
            assert torch.equal(got.cpu().float().nan_to_num(nan=-1.0), wanted.to(dtype).float().nan_to_num(nan=-1.0)), (rows, width)
            assert bool((guard[rows * width:] == -7.0).all())
            if rows == 33 and width == 33:
                nan = torch.zeros(rows, width, dtype=torch.bool)
                nan[32, 7] = True
                assert torch.equal(got.cpu().isnan(), nan)
