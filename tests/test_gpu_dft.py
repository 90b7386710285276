"""The sampled Fourier transform on the GPU (fewbit_hipx_sampled_dft of the companion library libfewbit_hipx.so,
fewbit_amd/csrc/fewbit_dft.hip) and the layer's 'dft' estimator on it.

Against numpy's float64 FFT of the same data on the host, `fft(m, axis=0, norm='ortho')[idx] * scale`.  The kernel computes in fp32
(four-step FFT, ~log2(rows) roundings), so, as in tests/test_gpu_dct.py:

    fp32 result              |err| <= 3e-6 * max|y|
    bf16 / fp16 result       |err| <= 2^-8 |y| / 2^-11 |y| + 3e-6 * max|y|       (one rounding of the fp32 result to the 16-bit dtype)

The inputs are multiples of 1/16 below 4 in magnitude: exact in all three dtypes, so one float64 reference serves every dtype.
"""
import numpy as np
import pytest
import torch

import fewbit
from fewbit_amd import cabi, cabi_x, linear
from helpers import BASE, captured_step_replays_fresh_rows, large_tile_capture_in_a_fresh_process

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
REL = {torch.float32: 0.0, torch.float16: 2.0**-11, torch.bfloat16: 2.0**-8}
DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def _data(rows, width, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-64, 64, (rows, width), generator=g).double() / 16.0


def close(got, want, dtype):
    """got: the (2, p, features) planes; want: complex (p, features)"""
    want = torch.as_tensor(np.stack([want.real, want.imag]), dtype=torch.float64)
    err = (got.detach().cpu().double() - want).abs()
    tol = REL[dtype] * want.abs() + 3e-6 * float(want.abs().max())
    return bool((err <= tol).all()), float((err / tol.clamp_min(1e-300)).max())


# (rows, features, padding of the leading dimension): every row family, odd / ragged / wide feature counts (the wide ones at small rows)
CASES = [(256, 770, 2), (256, 1, 1), (4096, 65, 3), (16384, 63, 1), (1 << 17, 3, 1), (768, 770, 6), (12288, 1, 3), (49152, 3, 5),
         (1280, 65, 2), (20480, 64, 8), (40960, 1, 1)]


@pytest.mark.parametrize('rows,features,pad', CASES)
def test_every_row_family_dtype_and_out_dtype_against_numpy(rows, features, pad):
    """p random rows with duplicates plus the corner rows 0, N/2, 1, N-1; fp32 / fp16 / bf16 input, result in fp32 and in the input's dtype;
    a leading dimension larger than the feature count"""
    wide = _data(rows, features + pad, rows + features)
    g = torch.Generator().manual_seed(features)
    idx = torch.cat([torch.randint(0, rows, (min(rows, 2000), ), generator=g), torch.tensor([0, rows // 2, 1, rows - 1, 0, rows // 2])])
    scale = 2.5
    want = np.fft.fft(wide[:, :features].numpy(), axis=0, norm='ortho')[idx.numpy()] * scale
    idx = idx.to(DEV)
    for dtype in DTYPES:
        x = wide.to(dtype).to(DEV)[:, :features]
        assert x.stride(0) == features + pad
        assert 'fewbit_hipx_sampled_dft' in linear.sampled_transform_path('dft', x)
        for out_dtype in (torch.float32, dtype):
            y = cabi_x.sampled_dft(x, idx, scale, out_dtype=out_dtype)
            assert y.shape == (2, idx.numel(), features) and y.dtype == out_dtype and y.is_contiguous()
            ok, worst = close(y, want, out_dtype)
            assert ok, (rows, features, dtype, out_dtype, worst)


def test_every_row_once_scale_and_caller_buffers():
    """p = rows (every k once, shuffled); caller-provided out and workspace; the layer-level entry returns complex64"""
    for rows in (256, 768, 1280, 4096, 32768):
        wide = _data(rows, 66 + 4, rows)
        g = torch.Generator().manual_seed(rows)
        idx = torch.randperm(rows, generator=g)
        want = np.fft.fft(wide[:, 2:68].numpy(), axis=0, norm='ortho')[idx.numpy()] * 0.5
        x = wide.float().to(DEV)[:, 2:68]
        ws = torch.empty(cabi_x.sampled_dft_workspace_bytes(rows, 66, rows, torch.float32), dtype=torch.uint8, device=DEV)
        out = torch.full((2, rows, 66), float('nan'), device=DEV)
        y = cabi_x.sampled_dft(x, idx.to(DEV), 0.5, out=out, workspace=ws)
        assert y.data_ptr() == out.data_ptr()
        ok, worst = close(y, want, torch.float32)
        assert ok, (rows, worst)
    # linear.sampled_transform keeps its contract: complex64 (p, features), the fp32 planes of the rows of `seed`
    x = _data(1024, 40, 5).to(torch.bfloat16).to(DEV)
    z = linear.sampled_transform('dft', x, 100, torch.Generator(device=DEV), seed=77, scale=3.0)
    planes = cabi_x.sampled_dft_seeded(x, 100, 77, 3.0, out_dtype=torch.float32)
    assert z.dtype == torch.complex64 and z.shape == (100, 40)
    assert torch.equal(z.real, planes[0]) and torch.equal(z.imag, planes[1])


def test_exact_zeros_conjugate_pairs_seeded_equals_explicit_and_repeats():
    """imaginary plane exactly 0 at k = 0 and k = N/2; sampled pairs k, N - k exact conjugates; the seeded call equals the explicit call on
    cabi.sampled_rows(seed) bit for bit (seed by value and as a device word); two calls are bit-identical whatever the workspace holds"""
    for n, rows in enumerate((1024, 768, 1280, 1 << 17, 262144)):
        for dtype in DTYPES:
            x = _data(rows, 66, n).to(dtype).to(DEV)
            g = torch.Generator().manual_seed(n)
            ks = torch.randint(1, rows // 2, (300, ), generator=g)
            idx = torch.cat([torch.tensor([0, rows // 2]), ks, rows - ks, torch.tensor([0])]).to(DEV)
            for out_dtype in (torch.float32, dtype):
                re, im = cabi_x.sampled_dft(x, idx, 1.5, out_dtype=out_dtype)
                assert bool((im[0] == 0).all() and (im[1] == 0).all() and (im[-1] == 0).all()), (rows, dtype, out_dtype)
                a, b = slice(2, 302), slice(302, 602)
                assert torch.equal(re[a], re[b]) and torch.equal(im[a], -im[b]), (rows, dtype, out_dtype)
                assert float(im[a].abs().max()) > 0
    cases = [(256, 40, 9000), (512, 66, 2047), (16384, 768, 3276), (65536, 32, 13107), (131072, 64, 26214), (262144, 70, 5000),
             (768, 40, 9000), (12288, 768, 2457), (49152, 32, 9830), (1280, 40, 9000), (20480, 130, 4096), (40960, 32, 8192)]
    for n, (rows, features, p) in enumerate(cases):
        dtype = DTYPES[n % 3]
        x = _data(rows, features, n).to(dtype).to(DEV)
        seed = 0x9e3779b97f4a7c15 * (n + 1) & 0xffffffffffffffff
        want = cabi_x.sampled_dft(x, cabi.sampled_rows(seed, rows, p).to(DEV), 0.5)
        assert torch.equal(cabi_x.sampled_dft_seeded(x, p, seed, 0.5), want), (rows, features, p)
        word = torch.tensor([seed - (1 << 64) if seed >= 1 << 63 else seed], dtype=torch.int64, device=DEV)
        assert torch.equal(cabi_x.sampled_dft_seeded(x, p, word, 0.5), want), (rows, features, p)
        need = cabi_x.sampled_dft_workspace_bytes(rows, features, p, dtype)
        dirty = torch.randint(0, 256, (need, ), dtype=torch.uint8, device=DEV)
        assert torch.equal(cabi_x.sampled_dft_seeded(x, p, seed, 0.5, workspace=dirty), want)
        assert torch.equal(cabi_x.sampled_dft_seeded(x, p, seed, 0.5, workspace=torch.full((need, ), 255, dtype=torch.uint8, device=DEV)), want)


def test_shapes_without_a_kernel_are_refused_by_name_and_keep_the_torch_fft_path():
    for rows in (48, 128, 384, 3000, 1792, 640, 81920, 98304, 524288):
        assert cabi_x.sampled_dft_workspace_bytes(rows, 64, 10) == 0
        x = torch.randn(rows, 8, device=DEV)
        idx = torch.zeros(4, dtype=torch.int64, device=DEV)
        with pytest.raises(cabi.FewbitHipError, match='rows'):
            cabi_x.sampled_dft(x, idx)
        with pytest.raises(cabi.FewbitHipError, match='rows'):
            cabi_x.sampled_dft_seeded(x, 4, 1)
        assert 'torch.fft' in linear.sampled_transform_path('dft', x)
    x = torch.randn(3000, 8, device=DEV)
    y = fewbit.functional.linear_grp(x, torch.randn(5, 8, device=DEV, requires_grad=True), None, proj_dim_ratio=0.2, matmul='dft')
    assert [t.dtype for t in y.grad_fn.saved_tensors] == [torch.complex64, torch.float32]           # torch.fft, as before
    with pytest.raises(cabi.FewbitHipError, match='out_dtype'):
        cabi_x.sampled_dft(torch.randn(256, 8, device=DEV).bfloat16(), torch.zeros(4, dtype=torch.int64, device=DEV), out_dtype=torch.float16)
    with pytest.raises(cabi.FewbitHipError, match='int64'):
        cabi_x.sampled_dft(torch.randn(256, 8, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV))
    assert cabi_x.sampled_dft(torch.randn(256, 8, device=DEV), torch.zeros(0, dtype=torch.int64, device=DEV)).shape == (2, 0, 8)
    prev = linear.use_native_sketch(False)
    try:
        assert 'torch.fft' in linear.sampled_transform_path('dft', torch.randn(1024, 8, device=DEV))
    finally:
        linear.use_native_sketch(prev)


@pytest.mark.parametrize('rows', (512, 768, 1280))
@pytest.mark.parametrize('three_d', (False, True))
@pytest.mark.parametrize('dtype', (torch.float32, torch.bfloat16))
def test_the_dft_layer_on_the_kernel_equals_the_torch_formulation_on_the_same_rows(dtype, three_d, rows, monkeypatch):
    """linear_grp(matmul='dft') with `_draw_seed` pinned samples cabi.sampled_rows(seed, rows, p); the torch.fft formulation is handed the
    SAME rows.  Forward, input and bias gradients are exact on both paths; the weight gradient agrees to 2e-5 (fp32: two fp32 FFTs) or
    3e-2 (bf16: the kernel path keeps bf16 planes and multiplies on the bf16 pipe, the torch path keeps complex64) of its largest entry."""
    seed = 0x1234567890abcdef
    monkeypatch.setattr(linear, '_draw_seed', lambda generator: seed)
    g = torch.Generator().manual_seed(rows)
    x = torch.randn(rows // 128, 128, 40, generator=g).to(dtype).to(DEV)
    w = (torch.randn(24, 40, generator=g) * 0.3).to(dtype).to(DEV)
    b = torch.randn(24, generator=g).to(dtype).to(DEV)
    gy = torch.randn(rows // 128, 128, 24, generator=g).to(dtype).to(DEV)
    if not three_d:
        x, gy = x.reshape(rows, 40), gy.reshape(rows, 24)
    assert 'fewbit_hipx_sampled_dft' in linear.sampled_transform_path('dft', x.reshape(-1, 40))
    grads = {}
    for native in (True, False):
        prev = linear.use_native_sketch(native)
        if not native:
            monkeypatch.setattr(linear, '_sampled_rows', lambda p, n, like, gen: cabi.sampled_rows(seed, n, p).to(like.device))
        try:
            xi, wi, bi = x.clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
            y = fewbit.functional.linear_grp(xi, wi, bi, proj_dim_ratio=0.25, matmul='dft')
            kept = [t for t in y.grad_fn.saved_tensors if t.data_ptr() != wi.data_ptr()]
            if native:                                       # two (p, features) planes of the layer's dtype, views of one buffer
                assert [(tuple(t.shape), t.dtype) for t in kept] == [((rows // 4, 40), dtype)] * 2
                assert kept[0].untyped_storage().data_ptr() == kept[1].untyped_storage().data_ptr()
            else:
                assert [t.dtype for t in kept] == [torch.complex64]
            y.backward(gy)
            grads[native] = (y.detach().float(), xi.grad.float(), bi.grad.float(), wi.grad.float())
        finally:
            linear.use_native_sketch(prev)
    for a, bb in zip(grads[True][:3], grads[False][:3]):
        assert torch.equal(a, bb)
    gw_n, gw_t = grads[True][3], grads[False][3]
    rel = float((gw_n - gw_t).abs().max() / gw_t.abs().max())
    assert rel <= (2e-5 if dtype == torch.float32 else 3e-2), rel


def test_the_seeded_dft_estimator_has_the_mean_and_spread_of_the_formulation_with_drawn_rows():
    """Over 3000 draws each, linear_grp(matmul='dft') on the kernel pair (rows of a seed) and on the torch.fft formulation (rows from randint)
    both average to the exact weight gradient (bias within 4 sigma), and their mean squared deviations from it agree within 5 % (standard
    error of the ratio ~ 2 %).  256 and 768 rows."""
    for rows in (256, 768):
        g = torch.Generator().manual_seed(rows)
        x = torch.randn(rows, 12, generator=g).to(DEV)
        w = (torch.randn(6, 12, generator=g) * 0.3).to(DEV)
        gy = torch.randn(rows, 6, generator=g).to(DEV)
        exact = gy.T @ x
        p, draws = rows // 4, 3000
        torch.manual_seed(9)
        msd = {}
        for native in (True, False):
            prev = linear.use_native_sketch(native)
            try:
                acc, dev2 = torch.zeros_like(exact, dtype=torch.float64), torch.zeros((), device=DEV, dtype=torch.float64)
                for _ in range(draws):
                    wi = w.clone().requires_grad_()
                    fewbit.functional.linear_grp(x, wi, None, proj_dim=p, matmul='dft').backward(gy)
                    acc += wi.grad
                    dev2 += ((wi.grad - exact) ** 2).sum()
                msd[native] = float(dev2) / draws
                bias = float(torch.linalg.norm(acc / draws - exact) / torch.linalg.norm(exact))
                spread = (msd[native] / draws) ** 0.5 / float(torch.linalg.norm(exact))
                assert bias <= 4.0 * spread + 1e-3, (rows, native, bias, spread)
            finally:
                linear.use_native_sketch(prev)
        print(f'\nseeded DFT estimator, {rows} rows: mean squared deviation kernel pair / torch formulation = {msd[True] / msd[False]:.4f}')
        assert abs(msd[True] / msd[False] - 1.0) <= 0.05, (rows, msd)


def test_a_captured_dft_layer_step_samples_fresh_rows_on_every_replay(monkeypatch):
    """The layer with matmul='dft' inside a hipGraph: the recorded seed kernel derives the seed of replay r from (the host draw made at capture
    time, the device counter); the replayed weight gradient equals the explicit product on cabi.sampled_rows of that seed, backward meets
    forward's rows, replays differ"""
    monkeypatch.setattr(linear, '_draw_seed', lambda generator: BASE)
    captured_step_replays_fresh_rows('dft', 512, 64, 96, torch.float32, 512)


def test_a_large_tile_shape_captures_after_a_warm_up_of_another_row_count():
    """32768 rows (LDS tiles above 64 KiB) captured in a fresh process whose only eager call was at 512 rows: the first call of a dtype
    reserves the LDS of every large-tile kernel of that dtype, so no attribute call falls inside the capture"""
    large_tile_capture_in_a_fresh_process('dft')


def test_the_layer_keeps_two_bf16_planes_and_its_forward_peak_is_workspace_plus_planes():
    """16384 x 3072 bf16 at ratio 0.2 (p = 3276): the saved tensors are two (p, 3072) bf16 planes; the forward adds at most the workspace,
    the planes, the layer's output and 1 MiB to the peak; the torch.fft path's peak is higher by at least the full complex64 transform"""
    rows, features, out_features = 16384, 3072, 768
    x = torch.randn(rows, features, device=DEV, dtype=torch.bfloat16)
    w = (torch.randn(out_features, features, device=DEV, dtype=torch.bfloat16) * 0.02).requires_grad_()
    p = linear.projection_dim(rows, 0.2)
    assert p == 3276
    planes_bytes = 2 * p * features * 2
    ws = cabi_x.sampled_dft_workspace_bytes(rows, features, p, torch.bfloat16)
    y_bytes = rows * out_features * 2
    peaks = {}
    for native in (True, False):
        prev = linear.use_native_sketch(native)
        try:
            fewbit.functional.linear_grp(x, w, None, proj_dim_ratio=0.2, matmul='dft')          # warm-up (library handles, GEMM workspace)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            m0 = torch.cuda.memory_allocated()
            y = fewbit.functional.linear_grp(x, w, None, proj_dim_ratio=0.2, matmul='dft')
            torch.cuda.synchronize()
            peaks[native] = torch.cuda.max_memory_allocated() - m0
            kept = [t for t in y.grad_fn.saved_tensors if t.data_ptr() != w.data_ptr()]
            if native:
                assert [(tuple(t.shape), t.dtype) for t in kept] == [((p, features), torch.bfloat16)] * 2
            del y, kept
        finally:
            linear.use_native_sketch(prev)
    print(f'\nforward peak above the input: kernel pair {peaks[True] / 2**20:.1f} MiB, torch.fft {peaks[False] / 2**20:.1f} MiB')
    assert peaks[True] <= ws + planes_bytes + y_bytes + (1 << 20), (peaks[True], ws, planes_bytes, y_bytes)
    assert peaks[False] - peaks[True] >= rows * features * 8, peaks
