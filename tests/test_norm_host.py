"""The normalized rows of a seed without a GPU (include/fewbit_hipx.h; fewbit_amd/csrc/fewbit_norm.hip): the six entry points of the companion
library (declared, exported, bound), the host evaluation of the state against an independent numpy restatement of the header's definition, its
identity with the packed form of a seed at whole groups, the size formula, the decode bound, the refusals before anything is launched, and
``fewbit.QuantizedLayerNorm`` on host tensors: the forward value, what is saved, the gradients on the saved codes, and the statistics of the
definition over 200 calls."""
import math
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fewbit_amd as fewbit
from fewbit_amd import cabi, cabi_x, norm
import norm_harness
from norm_harness import LAYER_NORM as KIND, M32, input_gradient_averages_out, order_keys, philox, saved_by, walk, walks, weight_gradient_is_unbiased

ROOT = Path(__file__).resolve().parents[1]
NORM_SYMBOLS = ('fewbit_hipx_norm_state_bytes', 'fewbit_hipx_norm_workspace', 'fewbit_hipx_norm_state_host', 'fewbit_hipx_norm_state_unpack_host',
                'fewbit_hipx_layer_norm_forward', 'fewbit_hipx_layer_norm_backward')
BITS = (2, 4, 8)
WIDTHS = (1, 3, 7, 8, 9, 63, 64, 65, 200, 770)
SEED = 0x1234567887654321
NAN_BITS = 0x7fc00000


# ---- the definition restated in numpy ----------------------------------------------------------------------------------------------------
def row_uniforms(r, width, seed):
    """U of the elements of row r: element 8 b + e takes the 16 bits of element e of block q = r * B + b, counter (q low, q high, 0, 7)"""
    blocks = (width + 7) // 8
    q = np.uint64(r * blocks) + np.arange(blocks, dtype=np.uint64)
    words = np.stack(philox(q & M32, q >> np.uint64(32), 0, 7, seed), axis=1)                  # blocks x 4
    i = np.arange(width)
    word = words[i >> 3, (i & 7) >> 1]
    u = np.where(i & 1, word >> np.uint64(16), word & np.uint64(0xffff))
    return u.astype(np.float32) / np.float32(65536)


def restated(xhat, bits, seed):
    """-> the state of the float32 matrix `xhat`, from the text of the header"""
    rows, width = xhat.shape
    levels = np.float32(2**bits - 1)
    blocks = (width + 7) // 8
    stride = (bits * blocks + 3) // 4 * 4
    params, code_bytes = [], bytearray()
    with np.errstate(all='ignore'):
        for r in range(rows):
            U = row_uniforms(r, width, seed)
            codes = np.zeros(8 * blocks, dtype=np.uint64)
            for first in range(0, width, 64):
                xs = xhat[r, first:first + 64]
                keys = order_keys(xs)
                lo, hi = xs[np.argmin(keys)], xs[np.argmax(keys)]
                span = np.float32(hi - lo)
                if not np.isfinite(xs).all() or not np.isfinite(span):
                    params += [NAN_BITS, NAN_BITS]
                    continue
                step = np.float32(span / levels)
                inv = np.float32(levels / span) if span > 0 else np.float32(0)
                if not np.isfinite(inv):
                    inv = np.float32(0)
                t = ((xs - lo).astype(np.float32) * inv).astype(np.float32)
                s = (t + U[first:first + 64]).astype(np.float32)
                codes[first:first + xs.size] = np.minimum(np.floor(s), levels).astype(np.uint64)
                params += [int(np.array(lo).view(np.uint32)), int(np.array(step).view(np.uint32))]
            row = bytearray()
            for block in codes.reshape(-1, 8):
                row += sum(int(c) << (bits * j) for j, c in enumerate(block)).to_bytes(bits, 'little')
            code_bytes += row + bytes(stride - len(row))
    return np.frombuffer(np.array(params, dtype='<u4').tobytes() + bytes(code_bytes), dtype=np.uint8)


def draw(rows, width, kind, salt=0):
    g = torch.Generator().manual_seed(91 + salt)
    if kind == 'normal':
        return torch.randn(rows, width, generator=g)
    if kind == 'constant':
        return torch.zeros(rows, width)
    if kind == 'poisoned':                                              # one NaN row (every group of it), the others clean
        x = torch.randn(rows, width, generator=g)
        x[rows // 2] = float('nan')
        return x
    raise KeyError(kind)


def steps_of(state, rows, width):
    """the step of every element's group, rows x width"""
    groups = (width + 63) // 64
    return state[:8 * rows * groups].view(torch.float32).view(rows, groups, 2)[:, :, 1].repeat_interleave(64, dim=1)[:, :width]


# ---- the library: symbols, sizes, the definition ------------------------------------------------------------------------------------------
def test_the_six_symbols_are_exported_declared_and_bound_and_the_revision_stays():
    header = (ROOT / 'include' / 'fewbit_hipx.h').read_text()
    declared = set(re.findall(r'\b(fewbit_hipx_\w+)\s*\(', header))
    out = subprocess.run(['nm', '-D', '--defined-only', str(cabi_x.LIB_PATH)], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in NORM_SYMBOLS:
        assert name in declared and name in exported and name in cabi_x.SYMBOLS, name
    assert declared == set(cabi_x.SYMBOLS) == {name for name in exported if name.startswith('fewbit_hipx_')}
    assert cabi_x.lib().fewbit_hipx_revision() == cabi_x.REVISION == 2 and cabi_x.lib().fewbit_hipx_abi_version() == cabi_x.ABI_VERSION == 1
    assert '#define FEWBIT_HIPX_REVISION 2' in header and 'The normalized rows of a seed.' in header


def test_state_bytes_is_the_formula():
    for bits in BITS:
        for rows in (1, 5, 16384):
            for width in WIDTHS + (768, 8192):
                blocks, groups = math.ceil(width / 8), math.ceil(width / 64)
                want = 8 * rows * groups + rows * (math.ceil(bits * blocks / 4) * 4)
                assert cabi_x.norm_state_bytes(rows, width, bits) == want, (rows, width, bits)
        assert cabi_x.norm_state_bytes(0, 64, bits) == 0 and cabi_x.norm_state_bytes(4, 0, bits) == 0 and cabi_x.norm_state_bytes(4, 8193, bits) == 0
        assert cabi_x.norm_state_bytes(2**36 // 64 + 1, 64, bits) == 0 and cabi_x.norm_state_bytes(2**36 // 64, 64, bits) != 0
        assert cabi_x.norm_state_bytes(-1, 64, bits) == 0
    for bits in (0, 1, 3, 5, 16):
        assert cabi_x.norm_state_bytes(4, 64, bits) == 0, bits
    # relative to a bf16 input, whole groups: the table of the documents; plus 4 bytes of rstd per row
    assert [cabi_x.norm_state_bytes(16384, 768, b) / (2 * 16384 * 768) for b in BITS] == [0.1875, 0.3125, 0.5625]
    # the workspace: one row of two padded columns sets per backward workgroup
    for width, rows, want in ((8, 1, 1 * 2 * 64 * 4), (8, 10**6, 512 * 2 * 64 * 4), (768, 16384, 512 * 2 * 1024 * 4), (8192, 3, 3 * 2 * 8192 * 4)):
        assert cabi_x.norm_workspace_bytes(rows, width) == want, (rows, width)
    assert cabi_x.norm_workspace_bytes(0, 8) == 0 and cabi_x.norm_workspace_bytes(4, 8193) == 0
    assert [cabi_x.norm_plan(w) for w in (64, 65, 128, 129, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097, 8192)] == [
        (8, 1), (16, 1), (16, 1), (64, 1), (64, 1), (128, 1), (128, 1), (256, 1), (256, 1), (256, 2), (256, 2), (256, 4), (256, 4)]


def test_the_walks_of_the_gpu_tests_begin_where_the_tables_say_and_rotate_over_every_dtype_and_code_width():
    """norm_harness.walk / walks, which tests/test_gpu_norm.py, test_gpu_rms_norm.py and test_gpu_add_norm.py stand on: the row counts are the ones
    written out here; a backward walk is refused by the helper where the library's workspace query says the grid is not at its cap; and the
    plain cases of either kind hold every (plan, dtype) and (plan, bits) pair, every width and every sweep"""
    assert [walk(w, 'backward', t, e) for w, t, e in ((72, 2, 1), (128, 3, 1), (136, 2, 1), (192, 3, 1), (1032, 2, 1), (2048, 3, 1), (2048, 3, None), (2056, 2, 1),
                                                      (4096, 3, 1), (4096, 3, None), (4104, 2, 1), (4097, 3, 1), (8192, 3, None))] == [
        32769, 65537, 8193, 16385, 2049, 4097, 3 * 2048, 1025, 2049, 3 * 1024, 513, 1025, 3 * 512]
    assert [walk(w, 'forward', t, 1) for w, t in ((128, 2), (192, 2), (136, 2), (1088, 2), (1032, 3), (2112, 2), (4160, 2))] == [
        16 * 16384 + 1, 4 * 16384 + 1, 4 * 16384 + 1, 16384 + 1, 2 * 16384 + 1, 16384 + 1, 16384 + 1]
    for width, tiles, extra in ((2048, 1, 1), (2048, 2, 0), (2048, 2, 2049)):
        with pytest.raises(AssertionError):
            walk(width, 'backward', tiles, extra)
    for direction, plans, widths in (('backward', 5, 11), ('forward', 5, 7)):
        for shift in (0, 1):
            cases = list(walks(direction, shift))
            assert all(c.rows(direction) > 0 for c in cases)
            assert len({(c.lanes, c.blocks) for c in cases}) == plans and len({c.width for c in cases}) == widths
            dtypes, bits = {(c.lanes, c.blocks, c.dtype) for c in cases}, {(c.lanes, c.blocks, c.bits) for c in cases}
            assert len(bits) == 3 * plans and len(dtypes) == 3 * plans - (direction == 'forward')      # (four blocks per lane: the two 16-bit dtypes)
            assert all(c.dtype != torch.float32 for c in cases if c.blocks == 4) and all(c.off == 1 for c in cases if c.width == 4097)
    assert len(list(walks('backward'))) == 29 and len(list(walks('forward'))) == 16
    assert {(c.width, c.tiles, c.extra) for c in walks('backward')} == {(w, t, e) for _, ws, sweeps in norm_harness.BACKWARD_WALKS for w in ws for t, e in sweeps}
    assert {(c.width, c.tiles, c.extra) for c in walks('forward')} == {(w, t, e) for _, ws, sweeps in norm_harness.FORWARD_WALKS for w in ws for t, e in sweeps}


@pytest.mark.parametrize('width', WIDTHS)
@pytest.mark.parametrize('bits', BITS)
def test_state_host_equals_the_definition_restated(bits, width):
    for rows in (1, 5):
        for kind in ('normal', 'constant', 'poisoned'):
            xhat = draw(rows, width, kind, width)
            for seed in (SEED, 7):
                got = cabi_x.norm_state_host(xhat, seed, bits)
                assert got.numel() == cabi_x.norm_state_bytes(rows, width, bits)
                want = restated(xhat.numpy(), bits, seed)
                assert np.array_equal(got.numpy(), want), (rows, kind, seed, np.flatnonzero(got.numpy() != want)[:8])
    if width >= 8:
        assert not torch.equal(cabi_x.norm_state_host(draw(5, width, 'normal'), 1, bits), cabi_x.norm_state_host(draw(5, width, 'normal'), 2, bits))


@pytest.mark.parametrize('width', (64, 768))
@pytest.mark.parametrize('bits', BITS)
def test_at_whole_groups_the_state_is_the_packed_form_of_the_flat_rows(bits, width):
    for rows in (1, 5):
        xhat = draw(rows, width, 'normal', 3)
        assert torch.equal(cabi_x.norm_state_host(xhat, SEED, bits), cabi_x.quant_pack_host(xhat.flatten(), SEED, bits))
        state = cabi_x.norm_state_host(xhat, SEED, bits)
        assert torch.equal(cabi_x.norm_state_unpack_host(state, rows, width, bits).flatten(), cabi_x.quant_unpack_host(state, rows * width, bits))


@pytest.mark.parametrize('bits', BITS)
def test_decode_is_within_one_step_of_every_element(bits):
    for rows, width in ((5, 200), (3, 770), (5, 7), (2, 65)):
        xhat = draw(rows, width, 'normal', 1)
        state = cabi_x.norm_state_host(xhat, SEED, bits)
        decoded = cabi_x.norm_state_unpack_host(state, rows, width, bits)
        step = steps_of(state, rows, width).double()
        err = (decoded.double() - xhat.double()).abs()
        print(f'bits {bits} {rows} x {width}: max |error| / step = {float((err / step.clamp_min(1e-300)).max()):.6f}')
        assert bool((err <= step * (1 + 2.0**-20)).all())
    constant = cabi_x.norm_state_host(torch.zeros(3, 70), SEED, bits)
    assert not bool(constant.any())                                   # x^ = 0: lo = step = +0 and every code 0
    poisoned = draw(5, 200, 'poisoned')
    decoded = cabi_x.norm_state_unpack_host(cabi_x.norm_state_host(poisoned, SEED, bits), 5, 200, bits)
    assert bool(torch.isnan(decoded[2]).all()) and not bool(torch.isnan(decoded[[0, 1, 3, 4]]).any())


def test_calls_are_refused_by_code_and_text_before_anything_is_launched():
    """(null and fake pointers throughout: a call that got as far as a launch would fail loudly)"""
    L = cabi_x.lib()
    err = lambda: L.fewbit_hipx_last_error().decode()
    fwd, bwd = L.fewbit_hipx_layer_norm_forward, L.fewbit_hipx_layer_norm_backward
    fake = 4096                                                       # an aligned non-null address that is never dereferenced
    ok_f = dict(dtype=2, x=fake, rows=4, width=64, gamma=fake, beta=fake, eps=1e-5, bits=4, seed=1, word=None, y=fake, rstd=fake, state=fake, size=2048,
                xhat=None, stream=None)
    ok_b = dict(dtype=2, gy=fake, state=fake, rstd=fake, gamma=fake, rows=4, width=64, bits=4, dx=fake, dgamma=fake, dbeta=fake, ws=fake, size=2**20, stream=None)
    f = lambda **kw: fwd(*{**ok_f, **kw}.values())
    b = lambda **kw: bwd(*{**ok_b, **kw}.values())
    assert f(dtype=3) == -1 and 'dtype 3' in err() and b(dtype=5) == -1 and 'dtype 5' in err()
    for bits in (0, 1, 3, 5, 16):
        assert f(bits=bits) == -1 and f'bits = {bits}' in err()
        assert b(bits=bits) == -1 and f'bits = {bits}' in err()
    for width in (0, 8193):
        assert f(width=width) == -1 and f'width = {width}' in err() and b(width=width) == -1 and f'width = {width}' in err()
    assert f(rows=2**36 // 64 + 1, size=2**40) == -1 and '2^36' in err() and b(rows=2**36 // 64 + 1) == -1 and '2^36' in err()
    assert f(x=None) == -1 and 'null' in err() and f(y=None) == -1 and 'null' in err() and f(rstd=None) == -1 and 'null' in err()
    assert b(gy=None) == -1 and 'null' in err() and b(state=None) == -1 and 'null' in err() and b(rstd=None) == -1 and 'null' in err()
    for name in ('x', 'y', 'gamma', 'beta'):
        assert f(**{name: fake + 1}) == -1 and 'element size' in err(), name
        assert f(dtype=0, **{name: fake + 2}) == -1 and 'element size' in err(), name
    for name in ('gy', 'dx', 'gamma'):
        assert b(**{name: fake + 1}) == -1 and 'element size' in err(), name
    assert f(rstd=fake + 2) == -1 and '4-byte' in err() and f(xhat=fake + 2) == -1 and '4-byte' in err()
    assert b(rstd=fake + 2) == -1 and '4-byte' in err() and b(dgamma=fake + 2) == -1 and '4-byte' in err() and b(dbeta=fake + 1) == -1 and '4-byte' in err()
    assert f(state=fake + 4) == -1 and '8-byte' in err() and b(state=fake + 4) == -1 and '8-byte' in err()
    need = cabi_x.norm_state_bytes(4, 64, 4)
    assert f(size=need - 1) == -1 and f'{need - 1} bytes, {need} are needed' in err()
    assert f(word=fake + 4) == -1 and 'seed word' in err()
    assert f(eps=-1.0) == -1 and 'eps' in err() and f(eps=float('nan')) == -1 and 'eps' in err()
    assert b(ws=None) == -1 and 'workspace' in err() and b(ws=fake + 8) == -1 and 'workspace' in err()
    need = cabi_x.norm_workspace_bytes(4, 64)
    assert b(size=need - 1) == -1 and f'{need - 1} bytes, {need} are needed' in err()
    # no rows, and a backward with no output: nothing to do, whatever the pointers
    assert f(rows=0, x=None, y=None) == 0 and b(rows=0, gy=None, state=None) == 0 and b(dx=None, dgamma=None, dbeta=None, ws=None, size=0) == 0
    # the host functions
    H, U = L.fewbit_hipx_norm_state_host, L.fewbit_hipx_norm_state_unpack_host
    assert H(None, 2, 8, 4, 1, fake) == -1 and 'null' in err() and H(fake, 2, 8, 3, 1, fake) == -1 and 'bits = 3' in err()
    assert H(fake, 2, 8193, 4, 1, fake) == -1 and 'width = 8193' in err() and U(fake, 2, 0, 4, fake) == -1 and 'width = 0' in err()
    assert U(fake, 2, 8, 4, None) == -1 and 'null' in err() and H(None, 0, 8, 4, 1, None) == 0 and U(None, 0, 8, 4, None) == 0


def test_the_binding_refuses_host_tensors_and_unknown_widths():
    with pytest.raises(cabi.FewbitHipError, match='GPU'):
        cabi_x.layer_norm_forward(torch.zeros(2, 8), None, None, 1e-5)
    with pytest.raises(cabi.FewbitHipError, match='GPU'):
        cabi_x.layer_norm_backward(torch.zeros(2, 8), torch.zeros(64, dtype=torch.uint8), torch.zeros(2), None, 4)
    for call in (lambda: cabi_x.norm_state_host(torch.zeros(2, 8), 1, 3), lambda: cabi_x.norm_state_unpack_host(torch.zeros(64, dtype=torch.uint8), 2, 8, 3)):
        with pytest.raises(cabi.FewbitHipError, match='bits must be 2, 4 or 8'):
            call()
    with pytest.raises(cabi.FewbitHipError, match='width = 8193'):
        cabi_x.norm_state_host(torch.zeros(1, 8193), 1, 4)
    with pytest.raises(cabi.FewbitHipError, match='at least 24 bytes'):
        cabi_x.norm_state_unpack_host(torch.zeros(23, dtype=torch.uint8), 2, 8, 4)
    assert cabi_x.norm_state_host(torch.zeros(0, 8), 1, 4).numel() == 0


# ---- fewbit.QuantizedLayerNorm on the host --------------------------------------------------------------------------------------------------
formula64, exact_rows = KIND.formula64, KIND.exact_rows          # (dx, dgamma, dbeta) and (x^, rstd) of the definition in float64


@pytest.mark.parametrize('bits', BITS)
@pytest.mark.parametrize('dtype', (torch.float32, torch.float64), ids=('float32', 'float64'))
def test_layer_on_host_tensors(dtype, bits):
    torch.manual_seed(3)
    width, rows = 200, 48
    layer = fewbit.QuantizedLayerNorm(width, dtype=dtype, bits=bits)
    with torch.no_grad():
        layer.weight.copy_(torch.randn(width) + 1)
        layer.bias.copy_(torch.randn(width))
    x = (3 + 2 * torch.randn(4, rows // 4, width)).to(dtype).requires_grad_()    # (three dimensions: the rows are the leading two)
    gy = torch.randn(4, rows // 4, width, dtype=dtype)
    y, saved = saved_by(lambda: layer(x))
    assert type(y.grad_fn).__name__ == '_LayerNormQuantizedBackward' and torch.equal(y, F.layer_norm(x, (width, ), layer.weight, layer.bias, layer.eps))
    # exactly codes (one per byte of the padded rows), lo, step, rstd and gamma
    groups = math.ceil(width / 64)
    assert [(t.dtype, t.numel()) for t in saved] == [(torch.uint8, rows * groups * 64), (dtype, rows * groups), (dtype, rows * groups), (dtype, rows), (dtype, width)]
    assert saved[4] is layer.weight or saved[4].data_ptr() == layer.weight.data_ptr()
    codes, lo, step, rstd, gamma = saved
    assert int(codes.max()) <= 2**bits - 1
    xq = torch.addcmul(lo.double()[:, None], codes.view(-1, 64).double(), step.double()[:, None]).view(rows, -1)[:, :width]
    xhat, rstd64 = exact_rows(x.detach().reshape(rows, width), layer.eps)
    assert bool(((xq - xhat).abs() <= step.double().view(rows, groups).repeat_interleave(64, dim=1)[:, :width] * (1 + 1e-6) + 1e-6).all())
    gx, gw, gb = torch.autograd.grad(y, (x, layer.weight, layer.bias), gy)
    assert gx.shape == x.shape and gx.dtype == gw.dtype == gb.dtype == dtype
    if dtype == torch.float64:                                        # float64 arithmetic only: the formula on the saved codes
        dx, dgamma, dbeta = formula64(gy.reshape(rows, width), xq, rstd, gamma)
        for got, want in ((gx.reshape(rows, width), dx), (gw, dgamma), (gb, dbeta)):
            assert bool(((got - want).abs() <= 1e-12 * want.abs().clamp_min(1.0)).all())
        assert bool(((rstd - rstd64).abs() <= 1e-12 * rstd64).all())


def test_layer_arguments_repr_and_exports():
    for bits in (0, 1, 3, 5, 16):
        with pytest.raises(ValueError, match='bits should be 2, 4 or 8'):
            fewbit.QuantizedLayerNorm(4, bits=bits)
        with pytest.raises(ValueError, match='bits should be 2, 4 or 8'):
            fewbit.functional.layer_norm_quantized(torch.zeros(2, 4), (4, ), bits=bits)
    m = fewbit.QuantizedLayerNorm(6, eps=1e-6, bits=8)
    assert isinstance(m, torch.nn.LayerNorm) and repr(m) == 'QuantizedLayerNorm((6,), eps=1e-06, elementwise_affine=True, bits=8)'
    assert fewbit.QuantizedLayerNorm(6).bits == 4 and fewbit.QuantizedLayerNorm(6).generator is None
    assert fewbit.QuantizedLayerNorm is norm.QuantizedLayerNorm and fewbit.functional.layer_norm_quantized is norm.layer_norm_quantized
    import fewbit as alias
    assert alias.QuantizedLayerNorm is norm.QuantizedLayerNorm and alias.functional.layer_norm_quantized is norm.layer_norm_quantized
    assert {'QuantizedLayerNorm', 'layer_norm_quantized'} <= set(norm.__all__)
    assert 'QuantizedLayerNorm' not in fewbit.modules.__all__ and 'layer_norm_quantized' not in fewbit.modules.__all__
    # map_module swaps the norms of a built model; the parameters are shared
    model = torch.nn.Sequential(torch.nn.LayerNorm(4), torch.nn.Linear(4, 8), torch.nn.Sequential(torch.nn.LayerNorm(8, elementwise_affine=False)),
                                fewbit.QuantizedLayerNorm(8, bits=8)).eval()
    weight, bias = model[0].weight, model[0].bias
    model = fewbit.map_module(model, lambda m, path: fewbit.QuantizedLayerNorm.from_layer_norm(m, bits=2) if type(m) is torch.nn.LayerNorm else m)
    swapped = [m for m in model.modules() if type(m) is fewbit.QuantizedLayerNorm]
    assert [m.bits for m in swapped] == [2, 2, 8] and swapped[0].weight is weight and swapped[0].bias is bias and swapped[1].weight is None
    assert not swapped[0].training and swapped[0].eps == 1e-5 and swapped[0].normalized_shape == (4, )
    x = torch.randn(5, 4, requires_grad=True)
    assert model(x).shape == (5, 8)
    # no affine parameters, a normalized shape of two dimensions
    x = torch.randn(3, 5, 6, requires_grad=True)
    y, saved = saved_by(lambda: fewbit.functional.layer_norm_quantized(x, (5, 6), bits=4))
    assert torch.equal(y, F.layer_norm(x, (5, 6))) and len(saved) == 4 and saved[0].numel() == 3 * 64
    (gx, ) = torch.autograd.grad(y, x, torch.randn(3, 5, 6))
    assert gx.shape == x.shape


def test_no_grad_and_nothing_that_requires_grad_keep_nothing_and_draw_nothing():
    layer = fewbit.QuantizedLayerNorm(24)
    x = torch.randn(12, 24, requires_grad=True)
    state = torch.get_rng_state()
    with torch.no_grad():
        y, saved = saved_by(lambda: layer(x))
    assert y.grad_fn is None and not saved and torch.equal(y, F.layer_norm(x, (24, ), layer.weight, layer.bias))
    layer.requires_grad_(False)
    y, saved = saved_by(lambda: layer(x.detach()))
    assert y.grad_fn is None and not saved
    y, saved = saved_by(lambda: layer.eval()(x.detach()))
    assert y.grad_fn is None and not saved
    y, saved = saved_by(lambda: layer.eval()(x))                     # eval with gradients: torch's exact layer norm, no codes, no seed
    assert 'Quantized' not in type(y.grad_fn).__name__ and not any(t.dtype == torch.uint8 for t in saved)
    assert torch.equal(torch.get_rng_state(), state)                 # and nothing was drawn


def test_the_generator_decides_the_rounding_and_checkpointing_reproduces_it():
    from torch.utils.checkpoint import checkpoint
    x, w, b = torch.randn(12, 70, requires_grad=True), torch.randn(70, requires_grad=True), torch.randn(70, requires_grad=True)
    gy = torch.randn(12, 70)

    def grads(generator=None):
        return torch.autograd.grad(fewbit.functional.layer_norm_quantized(x, (70, ), w, b, 1e-5, 2, generator), (x, w, b), gy)

    a, c = grads(torch.Generator().manual_seed(4)), grads(torch.Generator().manual_seed(4))
    assert all(torch.equal(p, q) for p, q in zip(a, c)) and not torch.equal(a[1], grads(torch.Generator().manual_seed(5))[1])
    torch.manual_seed(8)
    plain = grads()
    for reentrant in (False, True):
        torch.manual_seed(8)
        y = checkpoint(lambda t, weight, bias: fewbit.functional.layer_norm_quantized(t, (70, ), weight, bias, 1e-5, 2), x, w, b, use_reentrant=reentrant)
        x.grad = w.grad = b.grad = None
        y.backward(gy)
        assert all(torch.equal(p.grad, q) for p, q in zip((x, w, b), plain)), reentrant
    x.grad = w.grad = b.grad = None


# ---- the statistics of the definition: 200 calls, fp32 host tensors, seeds from torch.manual_seed(0) (norm_harness) ------------------------------
@pytest.mark.parametrize('bits', BITS)
@pytest.mark.parametrize('shape', ((48, 200), (32, 64), (40, 8)), ids=lambda s: 'x'.join(map(str, s)))
def test_the_weight_gradient_is_unbiased(shape, bits):
    weight_gradient_is_unbiased(KIND, shape, bits)


@pytest.mark.parametrize('bits', BITS)
@pytest.mark.parametrize('shape', ((48, 200), (24, 770)), ids=lambda s: 'x'.join(map(str, s)))
def test_the_input_gradient_averages_out_up_to_its_second_order_bias(shape, bits):
    input_gradient_averages_out(KIND, shape, bits)
