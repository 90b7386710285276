"""The zero-extended sampled transforms on the GPU: bit for bit the plain entry points on a zero-filled copy, float64 accuracy, nothing read
behind the last row, and the layer with use_row_extension() on."""
import numpy as np
import pytest
import torch

import fewbit_amd as fewbit
from fewbit_amd import cabi, cabi_x, linear
from helpers import BASE, GOLDEN

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
# (N', valid): the smallest row count of every family, even and odd bounds for Makhoul's map.  Their pass A tiles are N1 = 16 (256, 768, 1280,
# 2304, 3840) and N1 = 32 (3584) only; the first test adds 131072 = 512 x 256 (the tile above 64 KiB) outside this tuple.  N1 = 64, 128 and 256,
# and every other row count, are pinned bit for bit by tests/test_gpu_transform_splits.py, which runs all 38 counts of the dispatch table.
PAIRS = ((256, 1), (256, 2), (256, 129), (256, 255), (256, 256), (768, 700), (1280, 1025), (2304, 2100), (3584, 3101), (3840, 3700))


@pytest.fixture(autouse=True)
def _native():
    prev = linear.use_native_sketch(True)
    yield
    linear.use_native_sketch(prev)


def _data(rows, valid, features, ld, dtype, seed):
    """-> (x: the first `valid` rows of a rows x ld buffer, as a valid x features view; the zero-filled rows x features copy)"""
    g = torch.Generator().manual_seed(seed)
    base = (torch.randint(-64, 65, (rows, ld), generator=g).float() / 16).to(dtype).to(DEV)
    x = base[:valid, :features]
    padded = torch.zeros(rows, features, dtype=dtype, device=DEV)
    padded[:valid] = x
    return x, padded


def _idx(rows, p, seed):
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, rows, (p, ), generator=g)
    idx[:6] = torch.tensor([0, rows - 1, rows // 2, 1, 1, rows - 1])
    return idx.to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _both(kind, x, rows, idx, p, seed, scale):
    if kind == 'dct':
        return cabi_x.sampled_dct_zext(x, rows, idx, scale), cabi_x.sampled_dct_zext_seeded(x, rows, p, seed, scale)
    return cabi_x.sampled_dft_zext(x, rows, idx, scale), cabi_x.sampled_dft_zext_seeded(x, rows, p, seed, scale)


def _plain(kind, m, idx, p, seed, scale):
    if kind == 'dct':
        return cabi.sampled_dct(m, idx, scale), cabi.sampled_dct_seeded(m, p, seed, scale)
    return cabi_x.sampled_dft(m, idx, scale), cabi_x.sampled_dft_seeded(m, p, seed, scale)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('kind', ('dct', 'dft'))
def test_the_call_equals_the_plain_entry_point_on_a_zero_filled_copy_bit_for_bit(kind, dtype):
    """explicit idx and rows of a seed; widths 8, 70 (a full tile and an edge tile), 7 (odd) and 64 with ld > features; valid == rows is the
    plain entry point on x itself"""
    for n, (rows, valid) in enumerate(PAIRS):
        for features, ld in ((8, 8), (70, 70), (7, 7), (64, 72)):
            x, padded = _data(rows, valid, features, ld, dtype, 100 * n + features)
            p, seed = 40, 77 + n
            idx = _idx(rows, p, n)
            got = _both(kind, x, rows, idx, p, seed, 1.5)
            want = _plain(kind, padded, idx, p, seed, 1.5)
            for a, b, how in zip(got, want, ('idx', 'seeded')):
                assert torch.equal(_bits(a), _bits(b)), (kind, dtype, rows, valid, features, ld, how)
            if valid == rows:
                for a, b in zip(got, _plain(kind, x, idx, p, seed, 1.5)):
                    assert torch.equal(_bits(a), _bits(b))
    # the 128 KiB tile: 131072 = 512 x 256 rows, 70000 of them in memory
    x, padded = _data(131072, 70000, 8, 8, dtype, 5)
    idx = _idx(131072, 40, 5)
    for a, b in zip(_both(kind, x, 131072, idx, 40, 9, 1.0), _plain(kind, padded, idx, 40, 9, 1.0)):
        assert torch.equal(_bits(a), _bits(b))
    # full 64-feature tiles of a wide matrix with an odd leading dimension (16-bit rows then start at 2-byte boundaries)
    x, padded = _data(2304, 2100, 192, 201, dtype, 6)
    idx = _idx(2304, 40, 6)
    for a, b in zip(_both(kind, x, 2304, idx, 40, 9, 1.0), _plain(kind, padded, idx, 40, 9, 1.0)):
        assert torch.equal(_bits(a), _bits(b))
    # a base pointer that is only element-aligned: a column-offset view of a wider buffer (pass A's 16-byte loads start at odd elements)
    g = torch.Generator().manual_seed(7)
    base = (torch.randint(-64, 65, (2304, 72), generator=g).float() / 16).to(dtype).to(DEV)
    x = base[:2100, 1:65]
    padded = torch.zeros(2304, 64, dtype=dtype, device=DEV)
    padded[:2100] = x
    assert x.data_ptr() % 16 != 0 and x.stride(0) == 72
    for a, b in zip(_both(kind, x, 2304, idx, 40, 9, 1.0), _plain(kind, padded, idx, 40, 9, 1.0)):
        assert torch.equal(_bits(a), _bits(b))


@pytest.fixture(scope='module')
def golden():
    """tests/golden/sampled_dct_ref_zext.npz (gen_transform_zext_golden.py): per pair of PAIRS the int8 input of `valid` rows, the row
    numbers and the reference's float64 dct(., dim=0, norm='ortho')[idx] of the input followed by zero rows; read once"""
    z = np.load(GOLDEN / 'sampled_dct_ref_zext.npz')
    cases = []
    for i in range(int(z['cases'])):
        rows, valid = (int(v) for v in z[f'case{i}_rows_valid'])
        cases.append((rows, valid, z[f'case{i}_x_times_16'], z[f'case{i}_idx'], z[f'case{i}_y']))
    assert tuple((c[0], c[1]) for c in cases) == PAIRS
    return cases


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('kind', ('dct', 'dft'))
def test_the_result_is_the_float64_transform_of_the_padded_data(kind, dtype, golden):
    """the tolerance DESIGN section 6 states for the DCT: 3e-6 max|y|, plus one rounding of the result for a 16-bit dtype (2^-8 bf16, 2^-11
    fp16, relative to max|y| as well).  'dct': against the reference's own float64 result in the fixture; 'dft': against numpy float64 of
    the same data followed by zero rows (the inputs are exact in every dtype).  Every pair of PAIRS, 40 features, 48 samples."""
    for rows, valid, x8, k, y in golden:
        x = (torch.from_numpy(x8.astype(np.float32)) / 16).to(dtype).to(DEV)
        idx = torch.from_numpy(k).to(DEV)
        if kind == 'dct':
            want = y
            got = cabi_x.sampled_dct_zext(x, rows, idx).cpu().double().numpy()
        else:
            ref = np.zeros((rows, x8.shape[1]))
            ref[:valid] = x8.astype(np.float64) / 16
            full = np.fft.fft(ref, axis=0, norm='ortho')[k]
            want = np.stack([full.real, full.imag])
            got = cabi_x.sampled_dft_zext(x, rows, idx).cpu().double().numpy()
        top = float(np.abs(want).max())
        err = float(np.abs(got - want).max())
        tol = (3e-6 + {torch.float32: 0.0, torch.float16: 2.0**-11, torch.bfloat16: 2.0**-8}[dtype]) * top
        print(f'\n{kind} {dtype} {rows} rows, {valid} in memory: max error {err / top:.3g} of max|y|, tolerance {tol / top:.3g}')
        assert err <= tol, (kind, dtype, rows, valid, err / top)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('kind', ('dct', 'dft'))
def test_nothing_behind_the_last_row_is_read_and_nothing_around_the_result_is_written(kind, dtype):
    """x: the first `valid` rows of an N'-row buffer whose other rows, and whose padding behind the features, are NaN; the result goes into
    the middle of a buffer of a known pattern"""
    for rows, valid, features, ld in ((256, 129, 8, 12), (768, 700, 70, 75), (3584, 3101, 64, 70), (3840, 3700, 128, 130)):
        g = torch.Generator().manual_seed(rows + valid)
        clean = (torch.randint(-64, 65, (valid, features), generator=g).float() / 16).to(dtype).to(DEV)
        dirty = torch.full((rows, ld), float('nan'), dtype=dtype, device=DEV)
        dirty[:valid, :features] = clean
        idx = _idx(rows, 40, rows)
        planes = () if kind == 'dct' else (2, )
        call = cabi_x.sampled_dct_zext if kind == 'dct' else cabi_x.sampled_dft_zext
        want = call(clean, rows, idx)
        guard = 64
        pattern = {torch.float32: 123.0, torch.float16: 123.0, torch.bfloat16: 123.0}[dtype]
        buf = torch.full((want.numel() + 2 * guard, ), pattern, dtype=dtype, device=DEV)
        out = buf[guard:guard + want.numel()].view(*planes, 40, features)
        got = call(dirty[:valid, :features], rows, idx, out=out)
        assert got.data_ptr() == out.data_ptr()
        assert torch.equal(_bits(got), _bits(want)), (kind, dtype, rows, valid)
        assert not bool(torch.isnan(got.float()).any())
        assert bool((buf[:guard] == pattern).all()) and bool((buf[-guard:] == pattern).all())


@pytest.mark.parametrize('dtype', (torch.float32, torch.bfloat16))
@pytest.mark.parametrize('kind', ('dct', 'dft'))
@pytest.mark.parametrize('rows,features,outs', ((3000, 40, 5), (300, 8, 6)))
def test_the_layer_with_the_switch_on_runs_zero_extended(kind, dtype, rows, features, outs, monkeypatch):
    """3000 x 40 -> 5 (N' = 3072) and 300 x 8 (N' = 512, the ceiling of 300).  grad_weight equals the torch formulation on the padded
    tensors with the same rows (cabi.sampled_rows(seed, N', p)) and scale N' / p, to 2e-5 (fp32) or 3e-2 (bf16) of its largest entry (the
    tolerance of test_gpu_transform_rows.py's layer test); the saved tensors are p x features in the layer's dtype (two for 'dft'), no
    complex64; grad_input and grad_bias are exact; the same seed gives the same bits; with the switch off everything is as before."""
    seed = 0x1234567890abcdef
    big = cabi_x.sampled_rows_ceil(rows)
    assert big == {3000: 3072, 300: 512}[rows]
    g = torch.Generator().manual_seed(rows)
    x = torch.randn(rows, features, generator=g).to(dtype).to(DEV)
    w = (torch.randn(outs, features, generator=g) * 0.3).to(dtype).to(DEV)
    b = torch.randn(outs, generator=g).to(dtype).to(DEV)
    gy = torch.randn(rows, outs, generator=g).to(dtype).to(DEV)
    p = linear.projection_dim(rows, 0.25)

    def step():
        xi, wi, bi = x.clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
        y = fewbit.functional.linear_grp(xi, wi, bi, proj_dim_ratio=0.25, matmul=kind)
        saved = [t for t in y.grad_fn.saved_tensors if t.shape != w.shape or t.data_ptr() != wi.data_ptr()]
        y.backward(gy)
        return y.detach(), xi.grad, bi.grad, wi.grad, saved

    assert 'torch.fft' in linear.sampled_transform_path(kind, x)
    off = step()
    assert off[4][0].shape == (p, features) and (kind == 'dct' or off[4][0].dtype == torch.complex64)
    prev = linear.use_row_extension(True)
    try:
        path = linear.sampled_transform_path(kind, x)
        assert f'fewbit_hipx_sampled_{kind}_zext' in path and f'zero-extended to {big} rows' in path
        assert 'torch.fft' in linear.sampled_transform_path(kind, x.double()) and 'torch.fft' in linear.sampled_transform_path(kind, x.cpu())
        monkeypatch.setattr(linear, '_draw_seed', lambda generator: seed)
        y, gx, gb, gw, saved = step()
        again = step()
        assert len(saved) == (2 if kind == 'dft' else 1)
        for t in saved:
            assert t.dtype == dtype and t.shape == (p, features)
        assert torch.equal(y, torch.nn.functional.linear(x, w, b)) and torch.equal(gx, gy @ w) and torch.equal(gb, gy.sum(0))
        assert torch.equal(_bits(gw), _bits(again[3]))
        # the torch formulation on the padded tensors, the same rows, scale N' / p
        k = cabi.sampled_rows(seed, big, p).to(DEV)
        xp, gp = torch.zeros(big, features, device=DEV), torch.zeros(big, outs, device=DEV)
        xp[:rows], gp[:rows] = x.float(), gy.float()
        if kind == 'dct':
            sx, sg = linear.dct(xp, dim=0, norm='ortho')[k] * (big / p), linear.dct(gp, dim=0, norm='ortho')[k]
            want = sg.T @ sx
        else:
            sx, sg = torch.fft.fft(xp, dim=0, norm='ortho')[k] * (big / p), torch.fft.fft(gp, dim=0, norm='ortho')[k]
            want = sg.real.T @ sx.real + sg.imag.T @ sx.imag
        rel = float((gw.float() - want).abs().max() / want.abs().max())
        print(f'\nlayer {kind} {dtype} {rows} rows at {big}: weight gradient against the torch formulation on the padded tensors {rel:.3g}')
        assert rel <= (2e-5 if dtype == torch.float32 else 3e-2), rel
        # sampled_transform() takes the same path
        st = linear.sampled_transform(kind, x, p, torch.Generator(device=DEV), seed=seed, scale=big / p)
        assert float((st - sx).abs().max()) <= (1e-4 if dtype == torch.float32 else 2e-2) * float(sx.abs().max())
    finally:
        linear.use_row_extension(prev)
    monkeypatch.undo()
    assert 'torch.fft' in linear.sampled_transform_path(kind, x)
    assert step()[4][0].dtype == off[4][0].dtype


def test_a_matrix_of_4_gib_or_more_keeps_torch_fft_with_the_switch_on():
    """the zero-extended pass A addresses valid_rows x ld elements below 4 GiB (its C entry point refuses more); the layer does not route
    such a matrix to it: the path text and _native_transform_rows answer as with the switch off.  (The memory is only reserved.)"""
    prev = linear.use_row_extension(True)
    try:
        for shape, dtype in (((200000, 11008), torch.bfloat16), ((250000, 4608), torch.float32)):
            x = torch.empty(shape, dtype=dtype, device=DEV)
            assert x.numel() * x.element_size() >= 1 << 32
            for kind in ('dct', 'dft'):
                assert linear._native_transform_rows(kind, x) == 0
                assert 'torch.fft' in linear.sampled_transform_path(kind, x)
                # a narrow view of the wide rows spans as much
                assert linear._native_transform_rows(kind, x[:, :64]) == 0
                # fewer rows of it span less: the kernel pair
                assert linear._native_transform_rows(kind, x[:3000]) == 3072
            del x
    finally:
        linear.use_row_extension(prev)
    assert linear._zext_span_ok(0xfffffff0 // 16, 8, 2) and not linear._zext_span_ok(0xfffffff0 // 16 + 1, 8, 2)


def test_a_hundred_sequences_of_128_tokens_run_at_14336_rows():
    prev = linear.use_row_extension(True)
    try:
        layer = fewbit.RandomizedLinear(64, 32, proj_dim_ratio=0.2, matmul='dct', device=DEV, dtype=torch.bfloat16)
        x = torch.randn(100, 128, 64, device=DEV, dtype=torch.bfloat16, requires_grad=True)
        assert 'zero-extended to 14336 rows' in linear.sampled_transform_path('dct', x.reshape(-1, 64))
        layer(x).sum().backward()
        assert layer.weight.grad.shape == (32, 64) and bool(torch.isfinite(layer.weight.grad.float()).all())
    finally:
        linear.use_row_extension(prev)


@pytest.mark.parametrize('kind', ('dct', 'dft'))
def test_a_captured_step_at_3000_rows_samples_fresh_rows_on_every_replay(kind, monkeypatch):
    """one fwd + bwd step at 3000 rows (zero-extended to 3072) inside a hipGraph, warmed up eagerly: the seed word advances with every
    replay, each replay equals the explicit zero-extended products on the rows of its seed, and replays differ (the scheme of
    helpers.captured_step_replays_fresh_rows, whose explicit product is the plain call)"""
    monkeypatch.setattr(linear, '_draw_seed', lambda generator: BASE)
    rows, big, features, p, dtype = 3000, 3072, 64, 600, torch.float32
    prev = linear.use_row_extension(True)
    try:
        lin = fewbit.RandomizedLinear(features, 32, proj_dim=p, matmul=kind, bias=False, device=DEV, dtype=dtype)
        x = torch.randn(rows, features, device=DEV, dtype=dtype, requires_grad=True)
        wgt = torch.randn(rows, 32, device=DEV, dtype=dtype)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            xw = torch.randn(300, features, device=DEV, dtype=dtype, requires_grad=True)
            torch.autograd.grad((lin(xw) * torch.randn(300, 32, device=DEV, dtype=dtype)).sum(), lin.weight)
        torch.cuda.current_stream().wait_stream(side)
        counter = linear._replay_counter(torch.device(DEV))
        c0 = int(counter)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            gw, = torch.autograd.grad((lin(x) * wgt).sum(), lin.weight)
        seen = []
        for r in range(3):
            g.replay()
            torch.cuda.synchronize()
            assert int(counter) == c0 + r + 1
            idx = cabi.sampled_rows(cabi.mix_sketch_seed(BASE, c0 + r), big, p).to(DEV)
            if kind == 'dct':
                want = cabi_x.sampled_dct_zext(wgt, big, idx).T @ cabi_x.sampled_dct_zext(x.detach(), big, idx, big / p)
            else:
                gr, gi = cabi_x.sampled_dft_zext(wgt, big, idx)
                xr, xi = cabi_x.sampled_dft_zext(x.detach(), big, idx, big / p)
                want = gr.T @ xr + gi.T @ xi
            assert torch.allclose(gw, want, rtol=1e-4, atol=1e-3), (r, float((gw - want).abs().max()))
            seen.append(gw.clone())
        assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
    finally:
        linear.use_row_extension(prev)
