"""Both sampled-transform kernel pairs at 7 x 2^k (3584 .. 57344), 9 x 2^k (2304 .. 36864) and 15 x 2^k (3840 .. 30720) rows: the
radix-7 first stage of pass B (N2 = 112 / 224) and the repeated radix-3 and radix-3-then-5 first stages (N2 = 144 / 288, 240).

'dct' against the REFERENCE'S OWN `dct(x, dim=0, norm='ortho')[idx]` in float64 (tests/golden/sampled_dct_ref_{7x,9x,15x}.npz, generator:
tests/golden/gen_transform_rows_golden.py), 'dft' against numpy's float64 `fft(m, axis=0, norm='ortho')[idx]` of the same data.  The
tolerances are those of tests/test_gpu_dct.py and tests/test_gpu_dft.py:

    fp32 result              |err| <= 3e-6 * max|y|
    bf16 / fp16 result       |err| <= 2^-8 |y| / 2^-11 |y| + 3e-6 * max|y|       (one rounding of the fp32 result to the 16-bit dtype)

and, per feature column on structured inputs, the criterion of tests/test_gpu_transform_columns.py:

    |err| <= REL |want| + 4 max(E_ref, u log2 N) RMS_c  (+ 2^-24 for fp16 results)
"""
import math

import numpy as np
import pytest
import torch

import fewbit
from fewbit_amd import cabi, cabi_x, linear
from helpers import BASE, GOLDEN, captured_step_replays_fresh_rows, reference_error, transform_error_check, transform_input, transform_rows

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
REL = {torch.float32: 0.0, torch.float16: 2.0**-11, torch.bfloat16: 2.0**-8}
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
PATHS = {'dct': 'fewbit_hip_sampled_dct', 'dft': 'fewbit_hipx_sampled_dft'}
NEW_ROWS = sorted([7 << k for k in range(9, 14)] + [9 << k for k in range(8, 13)] + [15 << k for k in range(8, 12)])


def _close(got, want, dtype):
    """got: the result (for 'dft' its two planes); want: float64 (p, features), complex for 'dft'"""
    want = np.asarray(want)
    want = torch.as_tensor(np.stack([want.real, want.imag]) if np.iscomplexobj(want) else want, dtype=torch.float64)
    err = (got.detach().cpu().double() - want).abs()
    tol = REL[dtype] * want.abs() + 3e-6 * float(want.abs().max())
    return bool((err <= tol).all()), float((err / tol.clamp_min(1e-300)).max())


def _strided(x, pad, dtype):
    """host (rows, features) -> a device view of `dtype` with a leading dimension `pad` larger"""
    wide = torch.cat([x, x[:, :1].expand(-1, pad)], 1).to(dtype).to(DEV)
    view = wide[:, :x.shape[1]]
    assert view.stride(0) == x.shape[1] + pad and not (x.shape[1] > 1 and view.is_contiguous())
    return view


def _integers(rows, width, seed):
    """multiples of 1/16 below 4 in magnitude: exact in all three dtypes"""
    return torch.randint(-64, 64, (rows, width), generator=torch.Generator().manual_seed(seed)).double() / 16.0


@pytest.fixture(scope='module', params=('sampled_dct_ref_7x.npz', 'sampled_dct_ref_9x.npz', 'sampled_dct_ref_15x.npz'))
def ref(request):
    with np.load(GOLDEN / request.param) as z:
        return {k: z[k].copy() for k in z.files}


def test_the_fixtures_cover_every_new_row_count():
    seen = set()
    for name in ('sampled_dct_ref_7x.npz', 'sampled_dct_ref_9x.npz', 'sampled_dct_ref_15x.npz'):
        with np.load(GOLDEN / name) as z:
            seen |= {z[f'case{i}_x_times_16'].shape[0] for i in range(int(z['cases']))}
    assert sorted(seen) == NEW_ROWS


@pytest.mark.parametrize('dtype', DTYPES)
def test_sampled_dct_rows_equal_the_reference_run(ref, dtype):
    """every case of the three fixture files in every dtype: explicit idx (corner rows, the self-paired residue classes, a duplicate), a
    leading dimension 5 larger than the feature count, two calls bit for bit equal"""
    for i in range(int(ref['cases'])):
        x = _strided(torch.from_numpy(ref[f'case{i}_x_times_16'].astype(np.float64) / 16.0), 5, dtype)
        idx = torch.from_numpy(ref[f'case{i}_idx']).to(DEV)
        assert PATHS['dct'] in linear.sampled_transform_path('dct', x)
        y = cabi.sampled_dct(x, idx)
        assert y.shape == (idx.numel(), x.shape[1]) and y.dtype == dtype
        ok, worst = _close(y, ref[f'case{i}_y'], dtype)
        print(f'\ndct {tuple(x.shape)} {dtype}: worst err / bound {worst:.3g}')
        assert ok, (i, tuple(x.shape), dtype, worst)
        assert torch.equal(cabi.sampled_dct(x, idx), y), (i, tuple(x.shape), dtype)


# (rows, features, padding of the leading dimension): the smallest and the largest row count of each family, ragged and 1-wide
DFT_CASES = [(3584, 65, 2), (57344, 1, 1), (2304, 770, 6), (36864, 3, 5), (3840, 1, 3), (30720, 67, 1)]


@pytest.mark.parametrize('rows,features,pad', DFT_CASES)
def test_sampled_dft_rows_equal_numpy_float64(rows, features, pad):
    """2000 random rows with duplicates plus the corner rows; fp32 / fp16 / bf16 input, both planes, result in fp32 and in the input's dtype"""
    x = _integers(rows, features, rows + features)
    g = torch.Generator().manual_seed(features)
    idx = torch.cat([torch.randint(0, rows, (2000, ), generator=g), torch.tensor([0, rows // 2, 1, rows - 1, 0, rows // 2])])
    want = np.fft.fft(x.numpy(), axis=0, norm='ortho')[idx.numpy()] * 2.5
    idx = idx.to(DEV)
    for dtype in DTYPES:
        xd = _strided(x, pad, dtype)
        assert PATHS['dft'] in linear.sampled_transform_path('dft', xd)
        for out_dtype in (torch.float32, dtype):
            y = cabi_x.sampled_dft(xd, idx, 2.5, out_dtype=out_dtype)
            assert y.shape == (2, idx.numel(), features) and y.dtype == out_dtype and y.is_contiguous()
            ok, worst = _close(y, want, out_dtype)
            print(f'\ndft {rows} x {features} {dtype} -> {out_dtype}: worst err / bound {worst:.3g}')
            assert ok, (rows, features, dtype, out_dtype, worst)
            assert bool((y[1, -2:] == 0).all()) and bool((y[1, -6:-4] == 0).all())               # k = 0 and k = N / 2: imaginary part exactly 0


@pytest.mark.parametrize('kind', ('dct', 'dft'))
def test_the_seeded_call_is_the_explicit_call_on_the_rows_of_the_seed(kind):
    """bit for bit, one row count of each family (128 x 112, 128 x 144, 64 x 240), the seed by value and as a device word, p beyond 8000 too"""
    for n, (rows, features, p) in enumerate(((14336, 66, 2867), (18432, 40, 9000), (15360, 130, 3072))):
        dtype = DTYPES[n % 3]
        x = _integers(rows, features, n).to(dtype).to(DEV)
        seed = 0x9e3779b97f4a7c15 * (n + 1) & 0xffffffffffffffff
        idx = cabi.sampled_rows(seed, rows, p).to(DEV)
        word = torch.tensor([seed - (1 << 64) if seed >= 1 << 63 else seed], dtype=torch.int64, device=DEV)
        if kind == 'dct':
            want = cabi.sampled_dct(x, idx, 0.5)
            assert torch.equal(cabi.sampled_dct_seeded(x, p, seed, 0.5), want), (rows, features, p)
            assert torch.equal(cabi.sampled_dct_seeded(x, p, word, 0.5), want), (rows, features, p)
        else:
            want = cabi_x.sampled_dft(x, idx, 0.5)
            assert torch.equal(cabi_x.sampled_dft_seeded(x, p, seed, 0.5), want), (rows, features, p)
            assert torch.equal(cabi_x.sampled_dft_seeded(x, p, word, 0.5), want), (rows, features, p)
        assert float(want.float().abs().max()) > 0


@pytest.mark.parametrize('rows', (3584, 2304, 3840))
@pytest.mark.parametrize('kind', ('dct', 'dft'))
def test_every_row_of_the_transform(kind, rows):
    """p = rows, idx a permutation: every k once against the float64 transform of the same data on the host -- a wrong digit map of the new
    lengths cannot hide behind the sample"""
    x = _integers(rows, 66, rows)
    idx = torch.randperm(rows, generator=torch.Generator().manual_seed(rows))
    xd = _strided(x, 4, torch.float32)
    if kind == 'dct':
        want = (fewbit.fft.dct(x, dim=0, norm='ortho')[idx] * 2.5).numpy()
        y = cabi.sampled_dct(xd, idx.to(DEV), 2.5)
    else:
        want = np.fft.fft(x.numpy(), axis=0, norm='ortho')[idx.numpy()] * 2.5
        y = cabi_x.sampled_dft(xd, idx.to(DEV), 2.5)
    ok, worst = _close(y, want, torch.float32)
    print(f'\n{kind} every row of {rows}: worst err / bound {worst:.3g}')
    assert ok, (kind, rows, worst)


# ---- structured inputs, per feature column -----------------------------------------------------------------------------------------
STRUCTURED_ROWS = (7168, 4608, 7680)                        # 64 x 112, 32 x 144, 32 x 240: 56, 36 and 60 sequences of 128 tokens
STRUCTURED = ('pure tone', 'constant', 'mean 1000 sigma', 'white noise', 'partners')


def structured_input(family, kind, rows, features, dtype, seed):
    """helpers.transform_input, and 'constant': every column one value (1 .. 5, equal within a pair)"""
    if family != 'constant':
        return transform_input(family, kind, rows, features, dtype, seed)
    amp = (1.0 + (torch.arange(features) // 2) % 5).double()
    return amp.expand(rows, features).clone().to(dtype).double(), rows // 3 + 7


def _transform(kind, x):
    return fewbit.fft.dct(x, dim=0, norm='ortho') if kind == 'dct' else torch.fft.fft(x, dim=0, norm='ortho')


@pytest.mark.parametrize('rows', STRUCTURED_ROWS)
@pytest.mark.parametrize('kind', ('dct', 'dft'))
def test_structured_inputs_meet_the_per_column_bound(kind, rows):
    """a pure tone on a sampled bin, a constant, a mean of 1000 sigma (fp16: 100), white noise, and partner columns 2^20 apart (fp16: 2^6;
    judged per pair, its zero pair exactly zero); all three dtypes, both DFT out dtypes; rows 0, N/2, N-1, the tone's bins and 1000 random
    ones; 67 features behind a leading dimension of 70.  E_ref: torch's fp32 transform of the same data on the device.  (The fp32
    reference alone meets the criterion on these inputs on the host: every ratio finite and <= 1 by construction of E_ref.)"""
    features = 67
    for dtype in DTYPES:
        for family in STRUCTURED:
            pair = family == 'partners'
            x, k0 = structured_input(family, kind, rows, features, dtype, rows + features)
            idx = transform_rows(rows, k0, 1000, rows).to(DEV)
            xd = _strided(x, 3, dtype)
            xg = x.to(DEV)
            want = _transform(kind, xg)[idx]
            e_ref = reference_error(_transform(kind, xg.float())[idx], want, xg, pair)
            for out_dtype in ((dtype, ) if kind == 'dct' or dtype == torch.float32 else (torch.float32, dtype)):
                got = cabi.sampled_dct(xd, idx) if kind == 'dct' else cabi_x.sampled_dft(xd, idx, out_dtype=out_dtype)
                floor = 2.0**-24 if out_dtype == torch.float16 else 0.0
                ok, worst, ratio = transform_error_check(got, want, xg, e_ref, REL[out_dtype], pair, floor)
                print(f'\n{kind} {family:16s} rows {rows:6d} {str(dtype)[6:]:8s} -> {str(out_dtype)[6:]:8s} E_ref / (u log2 N) '
                      f'{e_ref / (2.0**-24 * math.log2(rows)):7.3f}  kernel / max(E_ref, u log2 N) {ratio:9.3g}  worst err / bound {worst:7.3g}')
                assert ok, (kind, family, rows, dtype, out_dtype, worst, ratio)
                if pair:
                    assert bool((got[..., 2:4] == 0).all()), (kind, rows, dtype, out_dtype)


# ---- the layer ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('batch', (28, 18, 30))
@pytest.mark.parametrize('dtype', (torch.float32, torch.bfloat16))
@pytest.mark.parametrize('kind', ('dct', 'dft'))
def test_the_layer_on_the_kernel_pair_equals_the_layer_on_torch_fft(kind, dtype, batch, monkeypatch):
    """linear_grp(matmul=kind) at 28 x 128 = 7 x 2^9, 18 x 128 = 9 x 2^8 and 30 x 128 = 15 x 2^8 tokens.  With `_draw_seed` pinned the native
    path samples cabi.sampled_rows(seed, rows, p); the torch.fft formulation is handed the SAME rows.  Forward, input and bias gradients
    are exact on both; the weight gradient agrees to 2e-5 (fp32) or 3e-2 (bf16: the two paths round the sampled rows at different points)
    of its largest entry"""
    seed = 0x1234567890abcdef
    monkeypatch.setattr(linear, '_draw_seed', lambda generator: seed)
    g = torch.Generator().manual_seed(batch)
    x = torch.randn(batch, 128, 40, generator=g).to(dtype).to(DEV)
    w = (torch.randn(24, 40, generator=g) * 0.3).to(dtype).to(DEV)
    b = torch.randn(24, generator=g).to(dtype).to(DEV)
    gy = torch.randn(batch, 128, 24, generator=g).to(dtype).to(DEV)
    assert PATHS[kind] in linear.sampled_transform_path(kind, x.reshape(-1, 40))
    grads = {}
    for native in (True, False):
        prev = linear.use_native_sketch(native)
        if not native:
            monkeypatch.setattr(linear, '_sampled_rows', lambda p, n, like, gen: cabi.sampled_rows(seed, n, p).to(like.device))
        try:
            xi, wi, bi = x.clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
            y = fewbit.functional.linear_grp(xi, wi, bi, proj_dim_ratio=0.25, matmul=kind)
            y.backward(gy)
            grads[native] = (y.detach().float(), xi.grad.float(), bi.grad.float(), wi.grad.float())
        finally:
            linear.use_native_sketch(prev)
    for a, bb in zip(grads[True][:3], grads[False][:3]):
        assert torch.equal(a, bb)
    gw_n, gw_t = grads[True][3], grads[False][3]
    rel = float((gw_n - gw_t).abs().max() / gw_t.abs().max())
    print(f'\nlayer {kind} {dtype} {batch} x 128 tokens: weight gradient, kernel pair against torch.fft {rel:.3g}')
    assert rel <= (2e-5 if dtype == torch.float32 else 3e-2), rel


@pytest.mark.parametrize('kind', ('dct', 'dft'))
def test_a_captured_layer_step_at_3584_rows_samples_fresh_rows_on_every_replay(kind, monkeypatch):
    """one fwd + bwd step at 3584 = 32 x 112 rows inside a hipGraph, warmed up eagerly at 512 rows: every replay equals the explicit product
    on cabi.sampled_rows of its seed, replays differ"""
    monkeypatch.setattr(linear, '_draw_seed', lambda generator: BASE)
    captured_step_replays_fresh_rows(kind, 3584, 64, 716, torch.float32, 512)
