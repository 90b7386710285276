"""The row blocks of a seed without a GPU (include/fewbit_hipx.h, "The row blocks of a seed"; fewbit_amd/csrc/fewbit_mxdef.h): the symbols, the size
formula, the refusals, the definition on the host form against a restatement in Python, the plan of ``mx_wgrad``, and ``linear_mx`` on host tensors."""
import math
import re
import subprocess
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

import fewbit
from fewbit_amd import cabi_x

ROOT = Path(__file__).resolve().parents[1]
NAMES = ('mx_bytes', 'mx_pack_host', 'mx_unpack_host', 'mx_pack', 'mx_unpack', 'mx_wgrad_workspace', 'mx_wgrad')
FORMATS = {'fp4': (4, 1, 0, 6.0), 'fp6': (6, 3, 0, 7.5), 'fp8': (8, 3, -6, 448.0)}          # bits, mantissa bits, exponent of the smallest normal, largest value
NAN = float('nan')


def value_of(code, format):
    bits, m, emin, _ = FORMATS[format]
    mag = code & (2**(bits - 1) - 1)
    if format == 'fp8' and mag == 0x7F:
        return NAN
    field, frac = mag >> m, mag & (2**m - 1)
    value = frac * 2.0**(emin - m) if field == 0 else (1 + frac / 2**m) * 2.0**(field - 1 + emin)
    return -value if code >> (bits - 1) else value


def buffer_of(codes, scales, format):
    """a buffer built by hand: ``codes`` [blocks][width][32] integers, ``scales`` [blocks][width] bytes"""
    bits = FORMATS[format][0]
    raw = bytearray(b for block in scales for b in block)
    raw += bytes(-len(raw) % 16)
    for block in codes:
        for cell in block:
            raw += sum(c << (bits * r) for r, c in enumerate(cell)).to_bytes(4 * bits, 'little')
    return torch.frombuffer(raw, dtype=torch.uint8)


def scales_of(packed, rows, width):
    return packed[:-(-rows // 32) * width].view(-1, width)


def test_the_symbols_are_declared_exported_and_bound_and_the_revision_is_still_2():
    header = (ROOT / 'include' / 'fewbit_hipx.h').read_text()
    out = subprocess.run(['nm', '-D', '--defined-only', str(cabi_x.LIB_PATH)], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in NAMES:
        assert re.search(rf'fewbit_hipx_{name}\s*\(', header) and f'fewbit_hipx_{name}' in exported and f'fewbit_hipx_{name}' in cabi_x.SYMBOLS
    assert cabi_x.lib().fewbit_hipx_revision() == cabi_x.REVISION == 2 and cabi_x.lib().fewbit_hipx_abi_version() == cabi_x.ABI_VERSION == 1
    assert {'MX_FORMATS', 'MX_WGRAD_TILE', 'mx_wgrad_serves', 'mx_wgrad_slices'} | set(NAMES) <= set(cabi_x.__all__)
    assert fewbit.MXLinear is fewbit.linear.MXLinear and fewbit.functional.linear_mx is fewbit.linear.linear_mx


@pytest.mark.parametrize('format', FORMATS)
def test_the_size_is_the_layout_formula(format):
    for rows, width in ((1, 1), (32, 16), (33, 17), (69, 64 + 5), (16384, 768)):
        blocks = -(-rows // 32)
        assert cabi_x.mx_bytes(rows, width, format) == -(-blocks * width // 16) * 16 + blocks * width * 4 * FORMATS[format][0]
    assert [cabi_x.mx_bytes(*e, format) for e in ((0, 5), (5, 0), (1, 2**23 + 1), (2**14, 2**23))] == [0] * 4 and cabi_x.mx_bytes(4, 4, 'fp5') == 0


P = 4096                                                                  # a pointer that is never followed: every call below is refused before a launch
PACK = dict(dtype=2, src=P, rows=40, width=24, ld=24, format=4, role=0, seed=1, word=None, out=P, out_bytes=10**6, stream=None)
UNPACK = dict(packed=P, packed_bytes=10**6, rows=40, width=24, format=4, dtype=2, out=P, stream=None)
WGRAD = dict(grad=P, grad_bytes=10**9, kept=P, kept_bytes=10**9, format=4, rows=4096, fin=32, fout=32, dtype=0, out=P, ws=P, ws_bytes=10**9, stream=None)
REFUSALS = [('mx_pack', PACK, change, text) for change, text in (
    (dict(dtype=99), 'unknown dtype'), (dict(role=2), 'role'), (dict(word=P + 4), 'seed word'), (dict(format=5), 'format'), (dict(width=2**23 + 1), '2^23'),
    (dict(rows=2**30, width=2**20, ld=2**20), '2^36'), (dict(src=None), 'null'), (dict(out=None), 'null'), (dict(ld=23), 'ld'), (dict(src=P + 1), 'src'),
    (dict(out=P + 8), '16-byte'), (dict(out_bytes=cabi_x.mx_bytes(40, 24, 'fp4') - 1), 'bytes'))]
REFUSALS += [('mx_unpack', UNPACK, change, text) for change, text in (
    (dict(dtype=99), 'unknown dtype'), (dict(format=7), 'format'), (dict(packed=None), 'null'), (dict(packed=P + 8), '16-byte'), (dict(out=P + 1), 'out'),
    (dict(packed_bytes=cabi_x.mx_bytes(40, 24, 'fp4') - 1), 'bytes'))]
REFUSALS += [('mx_wgrad', WGRAD, change, text) for change, text in (
    (dict(dtype=99), 'unknown dtype'), (dict(format=5), 'format'), (dict(rows=0), 'rows = 0'), (dict(format=8), 'no kernel'), (dict(fin=48), 'no kernel'),
    (dict(fout=16), 'no kernel'), (dict(kept=None), 'null'), (dict(grad=P + 8), '16-byte'), (dict(out=P + 4), '16-byte'),
    (dict(grad_bytes=cabi_x.mx_bytes(4096, 32, 'fp8') - 1), 'bytes'), (dict(kept_bytes=cabi_x.mx_bytes(4096, 32, 'fp4') - 1), 'bytes'), (dict(ws=None), 'null'),
    (dict(ws=P + 8), '16-byte'), (dict(ws_bytes=cabi_x.mx_wgrad_workspace(4096, 32, 32, 'fp4') - 1), 'bytes'))]


@pytest.mark.parametrize('name, base, change, text', REFUSALS)
def test_what_the_device_entry_points_refuse_before_anything_is_launched(name, base, change, text):
    assert cabi_x.mx_wgrad_workspace(4096, 32, 32, 'fp4') > 0
    rc = getattr(cabi_x.lib(), 'fewbit_hipx_' + name)(*{**base, **change}.values())
    assert rc != 0 and text in cabi_x.lib().fewbit_hipx_last_error().decode()


def test_what_the_host_functions_refuse():
    x, out, lib = torch.zeros(40, 24), torch.zeros(10**4, dtype=torch.uint8), cabi_x.lib()
    assert lib.fewbit_hipx_mx_pack_host(x.data_ptr(), 40, 24, 5, 0, 1, out.data_ptr()) != 0 and lib.fewbit_hipx_mx_pack_host(x.data_ptr(), 40, 24, 4, 3, 1, out.data_ptr()) != 0
    assert lib.fewbit_hipx_mx_pack_host(None, 40, 24, 4, 0, 1, out.data_ptr()) != 0 and lib.fewbit_hipx_mx_unpack_host(out.data_ptr(), 2**20, 2**20, 4, x.data_ptr()) != 0
    with pytest.raises(cabi_x.FewbitHipError):
        cabi_x.mx_unpack_host(out[:100], 40, 24, 'fp4')


@pytest.mark.parametrize('format', FORMATS)
def test_every_code_decodes_to_the_formats_value_times_the_scale(format):
    count = 2**FORMATS[format][0]
    width = max(count // 32, 1)
    codes = [[[(32 * j + r) % count for r in range(32)] for j in range(width)]]
    for byte in (127, 130, 20):
        got = cabi_x.mx_unpack_host(buffer_of(codes, [[byte] * width], format), 32, width, format)
        want = torch.tensor([[value_of((32 * j + r) % count, format) * 2.0**(byte - 127) for j in range(width)] for r in range(32)], dtype=torch.float64)
        assert torch.equal(got.double().nan_to_num(nan=-1.0), want.nan_to_num(nan=-1.0))


@pytest.mark.parametrize('k', (-120, -3, 0, 5, 100))
@pytest.mark.parametrize('format', FORMATS)
def test_the_scale_is_the_smallest_that_does_not_clip_and_representable_values_survive_every_seed(format, k):
    bits, m, emin, largest = FORMATS[format]
    top = torch.tensor(largest * 2.0**k, dtype=torch.float32)
    values = torch.tensor([value_of(c, format) for c in range(2**bits) if value_of(c, format) == value_of(c, format)], dtype=torch.float32)[:32] * 2.0**k
    x = torch.zeros(32, 3)
    x[:len(values), 0] = values
    x[5, 0], x[0, 1], x[0, 2] = top, torch.nextafter(top, torch.tensor(math.inf)), -torch.nextafter(top, torch.tensor(0.0))
    for seed in range(20):
        packed = cabi_x.mx_pack_host(x, seed, format)
        decoded = cabi_x.mx_unpack_host(packed, 32, 3, format)
        byte = max(127 + k, 0)
        assert scales_of(packed, 32, 3).tolist() == [[byte, max(byte + 1, 0), byte]] and torch.equal(decoded[:, 0], x[:, 0])
        # just above: between the two neighbours at the next scale (never clipped to the largest value of this one); just below: the largest or its neighbour
        assert float(top) <= float(decoded[0, 1]) <= float(top) * (1 + 2.0**-m) and float(top) * (1 - 2.0**-m) <= -float(decoded[0, 2]) <= float(top)


@pytest.mark.parametrize('format', FORMATS)
def test_zero_cells_the_short_last_block_and_poisoned_cells(format):
    x = torch.randn(33, 5, generator=torch.Generator().manual_seed(5))
    x[:, 1] = 0.0
    x[7, 2], x[32, 3] = NAN, -math.inf
    packed = cabi_x.mx_pack_host(x, 77, format)
    scales = scales_of(packed, 33, 5)
    assert scales[:, 1].tolist() == [0, 0] and scales[0, 2] == 0xFF and scales[1, 3] == 0xFF and int((scales == 0xFF).sum()) == 2
    decoded = cabi_x.mx_unpack_host(packed, 33, 5, format)
    nan = torch.zeros(33, 5, dtype=torch.bool)
    nan[:32, 2], nan[32, 3] = True, True
    assert torch.equal(decoded.isnan(), nan) and bool((decoded[:, 1] == 0).all())
    # rows beyond the matrix were packed as +0: the same buffer read as 64 rows
    assert cabi_x.mx_bytes(64, 5, format) == packed.numel() and bool((cabi_x.mx_unpack_host(packed, 64, 5, format)[33:, [0, 1, 2, 4]] == 0).all())
    # the last block's scale comes from its one row alone
    alone = cabi_x.mx_pack_host(x[32:], 1, format)
    assert torch.equal(scales_of(alone, 1, 5)[0], scales[1])


@pytest.mark.parametrize('role', ('kept', 'grad'))
@pytest.mark.parametrize('format', FORMATS)
def test_the_mean_of_the_decode_over_1000_seeds(format, role):
    """|mean(decode) - x| <= 5 step / (2 sqrt(1000)) on every element, step the spacing of the format around the element: step / 2 bounds the deviation
    of one draw (the criterion of tests/test_quant_host.py; 1000 seeds pass it here, the worst element 2.7 - 3.5 units off)"""
    bits, m, emin, largest = FORMATS[format]
    rows, width, seeds = 70, 24, 1000
    x = torch.randn(rows, width, generator=torch.Generator().manual_seed(11)) * torch.logspace(-3, 3, width, base=2.0)
    total = torch.zeros(rows, width, dtype=torch.float64)
    for seed in range(seeds):
        packed = cabi_x.mx_pack_host(x, 0xABCDEF0000 + seed, format, role)
        total += cabi_x.mx_unpack_host(packed, rows, width, format).double()
    scale = torch.exp2(scales_of(packed, rows, width).double() - 127).repeat_interleave(32, dim=0)[:rows]
    step = torch.exp2(torch.floor(torch.log2(x.double().abs() / scale)).clamp_min(emin) - m) * scale
    worst = float(((total / seeds - x.double()).abs() / (step / (2 * math.sqrt(seeds)))).max())
    print(f'{format} {role}: the worst element is {worst:.2f} units of step / (2 sqrt(seeds)) off')
    assert worst <= 5.0
    assert role == 'kept' or not torch.equal(packed, cabi_x.mx_pack_host(x, 0xABCDEF0000 + seeds - 1, format, 'kept'))


def test_the_predicate_the_plan_and_the_workspace_agree_and_the_workspace_is_capped():
    bm, bn, bk = cabi_x.MX_WGRAD_TILE
    for format in ('fp4', 'fp6'):
        for rows in (1, 31, 127, 128, 4096, 16384):
            for fin, fout in ((32, 32), (96, 160), (768, 3072), (4096, 11008), (2**22, 32)):
                assert cabi_x.mx_wgrad_serves(rows, fin, fout, format)
                slices, need = cabi_x.mx_wgrad_slices(rows, fin, fout), cabi_x.mx_wgrad_workspace(rows, fin, fout, format)
                assert need == (slices * fout * fin * 4 if slices > 1 else 0) and need <= rows * fin * 2 and slices <= -(-rows // bk)
    for rows, fin, fout, format in ((0, 32, 32, 'fp4'), (64, 48, 32, 'fp4'), (64, 32, 16, 'fp6'), (64, 32, 32, 'fp8'), (64, 2**23, 32, 'fp4'), (2**20, 2**20, 32, 'fp4')):
        assert not cabi_x.mx_wgrad_serves(rows, fin, fout, format) and cabi_x.mx_wgrad_workspace(rows, fin, fout, format) == 0
    assert cabi_x.mx_wgrad_slices(131, 32, 32) == 2 and cabi_x.mx_wgrad_slices(127, 32, 32) == 1


@pytest.mark.parametrize('format', ('fp4', 'fp6'))
def test_the_layer_on_host_tensors_keeps_the_host_form_and_multiplies_the_exact_gradient(format, monkeypatch):
    gen = torch.Generator().manual_seed(3)
    x, w, b = (torch.randn(s, generator=gen, requires_grad=True) for s in ((5, 9, 24), (40, 24), (40, )))
    gy = torch.randn(5, 9, 40, generator=gen)
    monkeypatch.setattr(fewbit.linear, '_draw_seed', lambda generator: 0x1234)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        y = fewbit.functional.linear_mx(x, w, b, format)
    want = torch.autograd.grad(F.linear(x, w, b), (x, b), gy)
    gx, gw, gb = torch.autograd.grad(y, (x, w, b), gy)
    packed = cabi_x.mx_pack_host(x.detach().reshape(-1, 24), 0x1234, format)
    assert torch.equal(y, F.linear(x, w, b)) and torch.equal(gx, want[0]) and torch.equal(gb, want[1])
    assert any(t.dtype == torch.uint8 and torch.equal(t, packed) for t in saved) and not any(t.shape == x.shape for t in saved)
    assert torch.equal(gw, gy.reshape(-1, 40).T @ cabi_x.mx_unpack_host(packed, 45, 24, format))
    with pytest.raises(ValueError):
        fewbit.functional.linear_mx(x, w, b, 'fp8')
    with pytest.raises(ValueError):
        fewbit.MXLinear(24, 40, format='e3m2')
    layer = fewbit.MXLinear(24, 40, format=format).eval()
    assert layer(x).grad_fn.name() != '_LinearMXBackward' and fewbit.functional.linear_mx(x, w.detach(), b, format).grad_fn.name() != '_LinearMXBackward'
