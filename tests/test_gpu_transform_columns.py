"""Both sampled-transform kernel pairs (fewbit_hip_sampled_dct, fewbit_amd/csrc/fewbit_dct.hip; fewbit_hipx_sampled_dft,
fewbit_amd/csrc/fewbit_dft.hip) per feature column, on structured inputs.

tests/test_gpu_dct.py and tests/test_gpu_dft.py bound every entry by 3e-6 x the largest output of the whole call, on white noise.  A
column with a large mean puts sqrt(N) x its RMS into row 0, and that figure then excuses every other entry.  Here each entry is held to
its own column:

    |err| <= REL |want| + 4 max(E_ref, u log2 N) RMS_c  (+ 2^-24 for fp16 results)

RMS_c is the RMS of the entry's input column (the transforms are orthonormal: the RMS of its output column).  want is the float64
transform of the same input, rounded to the kernel's dtype.  E_ref is the largest such normalised error of the fp32 reference on the same
data and rows, measured in the same run: fewbit.fft.dct(x.float(), dim=0, norm='ortho') and torch.fft.fft(x.float(), dim=0,
norm='ortho').  The factor 4 comes from the host model in tests/test_transform_error_model.py.  There a correct packed four-step stays
within 1.3 x the reference, and the smallest structural defect modelled, a bf16 intermediate, is 280 x.

The pair contract.  Features (2c, 2c + 1) are one complex column of the kernels, so the error of column c scales with the RMS of the pair
(c, c ^ 1), and a non-finite value reaches the partner column.  The torch.fft formulation keeps every column apart.  On partners 2^20
apart (2^6 in fp16) the per-pair measure meets the criterion; the per-column ratio is printed, not bounded.  Outside the pair, columns are
bit for bit independent of each other, of the leading-dimension padding and of the memory around `out`.

Measured on an MI355X (profiles/r07_transform_columns.txt): kernel / max(E_ref, u log2 N), the largest normalised error left after
the output rounding over that unit, worst over the input dtypes, fp32 results (the test asserts <= 4; the last line is the
per-column figure of the partner family, recorded, not bounded).  The closest to the bound is the DCT's pure tone at 2^14 rows, 3.48:
its largest error sits at bin N/2 - k0, where the tone leaks through the butterflies of the length-128 transforms; the library FFT of
the reference leaks less there.  A first version of these inputs gave the two columns of a pair different amplitudes, and the DCT's tone
then measured 5.2 at 3 x 2^12 rows: the pair contract, which the 'partners' family covers, so every other family keeps a pair equal:

    family            DCT 2^14  3x2^12  5x2^11    2^17    2^18   DFT 2^14  3x2^12  5x2^11    2^17    2^18
    white noise           0.90     0.91     0.98     0.77     1.13       0.65     0.85     0.74     0.64     0.60
    mean 1000 sigma       0.95     1.02     0.88     1.13     0.97       1.00     1.00     1.14     1.00     1.00
    random walk           0.81     1.17     0.60     1.82     1.06       1.33     1.57     1.02     1.00     1.12
    single spike          0.69     0.67     0.74     0.65     0.56       0.42     0.53     0.60     0.39     0.38
    pure tone             3.48     1.00     1.17     1.60     0.67       0.88     0.88     1.62     1.23     1.01
    alternating           1.00     1.71     1.00     1.00     1.00       0.00     1.00     1.00     1.00     0.00
    scales per pair       0.90     0.91     0.98     0.77     1.13       0.65     0.85     0.74     0.64     0.60
    partners              0.80     0.80     0.94     0.64     0.79       0.56     0.80     0.68     0.57     0.51
    partners, per col    5e+05  5.2e+05  4.7e+05  4.1e+05  4.3e+05    4.4e+05  4.3e+05  4.6e+05  3.8e+05  3.4e+05
"""
import math

import pytest
import torch

import fewbit
from fewbit_amd import cabi, cabi_x, linear
from helpers import TRANSFORM_FAMILIES, assert_bit_equal, bits, reference_error, transform_error_check, transform_input, transform_rows

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
REL = {torch.float32: 0.0, torch.float16: 2.0**-11, torch.bfloat16: 2.0**-8}
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
# one row count of each family: 2^k (128 x 128), 3 x 2^k (128 x 96), 5 x 2^k (64 x 160); the 512-point tiles 2^17, 2^18
ROWS = (16384, 12288, 10240, 1 << 17, 1 << 18)
PAD = 3


def _features(rows):
    """odd: a full tile and a partial one with a partnerless last column; one partial tile at 2^18 (rows x features <= 2^24)"""
    return 67 if rows <= 1 << 17 else 33


def _transform(kind, x):
    if kind == 'dct':
        return fewbit.fft.dct(x, dim=0, norm='ortho')
    return torch.fft.fft(x, dim=0, norm='ortho')


def _kernel(kind, x, idx, out_dtype):
    if kind == 'dct':
        return cabi.sampled_dct(x, idx)
    return cabi_x.sampled_dft(x, idx, out_dtype=out_dtype)


def _out_dtypes(kind, dtype):
    return (dtype, ) if kind == 'dct' or dtype == torch.float32 else (torch.float32, dtype)


def _on_device(x, dtype):
    """x (host float64, exact in dtype) as a (rows, features) view of dtype with a leading dimension PAD larger"""
    wide = torch.cat([x, x[:, :PAD]], 1).to(dtype).to(DEV)
    view = wide[:, :x.shape[1]]
    assert view.stride(0) == x.shape[1] + PAD
    return view


def _check(kind, family, rows, dtype, pair=False):
    """one case: every out dtype of the pair; -> [(out dtype, E_ref / (u log2 N), kernel / max(E_ref, u log2 N), per-column ratio)]"""
    features = _features(rows)
    x, k0 = transform_input(family, kind, rows, features, dtype, rows + features)
    idx = transform_rows(rows, k0, 1000, rows).to(DEV)
    xd = _on_device(x, dtype)
    xg = x.to(DEV)
    want = _transform(kind, xg)[idx]
    e_ref = reference_error(_transform(kind, xg.float())[idx], want, xg, pair)
    found = []
    for out_dtype in _out_dtypes(kind, dtype):
        got = _kernel(kind, xd, idx, out_dtype)
        floor = 2.0**-24 if out_dtype == torch.float16 else 0.0
        ok, worst, ratio = transform_error_check(got, want, xg, e_ref, REL[out_dtype], pair, floor)
        per_column = float('nan')
        if pair:
            _, _, per_column = transform_error_check(got, want, xg, e_ref, REL[out_dtype], False, floor)
        unit = e_ref / (2.0**-24 * math.log2(rows))
        print(f'\n{kind} {family:16s} rows {rows:6d} {str(dtype)[6:]:8s} -> {str(out_dtype)[6:]:8s} E_ref / (u log2 N) {unit:7.3f}  '
              f'kernel / max(E_ref, u log2 N) {ratio:9.3g}' + (f'  per column {per_column:9.3g}' if pair else '') + f'  worst err / bound {worst:7.3g}')
        assert ok, (kind, family, rows, dtype, out_dtype, worst, ratio)
        found.append((out_dtype, unit, ratio, per_column))
        if pair:                                                          # the zero pair (2, 3): exact zeros, by value (-0 counts)
            assert float(x[:, 2:4].abs().max()) == 0.0
            assert bool((got[..., 2:4] == 0).all()), (kind, rows, dtype, out_dtype)
    return found


@pytest.mark.parametrize('rows', ROWS)
@pytest.mark.parametrize('kind', ('dct', 'dft'))
def test_every_structured_family_meets_the_per_column_bound(kind, rows):
    """white noise, a mean of 1000 sigma (fp16: 100), a random walk, a single spike, a pure tone on a sampled bin, alternating +-1, scales
    2^-30 / 1 / 2^30 (fp16: 2^-6 / 1 / 2^6) per pair; all three input dtypes, both DFT out dtypes; sampled rows 0, N/2, N-1, the tone's
    bins and 1000 random ones; an odd feature count and a leading dimension 3 larger"""
    for dtype in DTYPES:
        for family in TRANSFORM_FAMILIES:
            _check(kind, family, rows, dtype)


@pytest.mark.parametrize('kind', ('dct', 'dft'))
def test_partner_columns_far_apart_meet_the_per_pair_bound_and_a_zero_pair_stays_zero(kind):
    """columns 2c and 2c + 1 2^20 apart (fp16: 2^6), the larger one alternating between them; the per-pair measure meets the criterion,
    the per-column ratio is recorded (the coupling of the packing); the all-zero pair (2, 3) gives exact zeros"""
    for rows in ROWS:
        for dtype in DTYPES:
            _check(kind, 'partners', rows, dtype, pair=True)


def _columns_of(kind, y):
    """-> (p, features) views of every plane of a result"""
    return (y, ) if kind == 'dct' else (y[0], y[1])


@pytest.mark.parametrize('kind', ('dct', 'dft'))
def test_a_non_finite_value_stays_in_its_pair(kind):
    """NaN, +Inf or -Inf at one entry of one column -- in a middle tile, in the last, partial tile and in the partnerless last column of an
    odd feature count: every column outside the pair (c, c ^ 1) is bit-identical to the call on the clean input; column c is non-finite in
    every sampled row, as in the reference run column by column on the host"""
    features = 195                                                     # tiles 0 .. 2 full, tile 3: features 192, 193, 194 (no 195)
    for rows in (4096, 3072, 1280):
        idx = transform_rows(rows, rows // 3 + 7, 300, rows)
        for dtype in DTYPES:
            clean, _ = transform_input('white noise', kind, rows, features, dtype, rows)
            xd = _on_device(clean, dtype)
            base = {o: _kernel(kind, xd, idx.to(DEV), o) for o in _out_dtypes(kind, dtype)}
            for row, col in ((rows // 3, 81), (5, 192), (rows - 1, 194)):
                pair = {col, col ^ 1} & set(range(features))
                others = [c for c in range(features) if c not in pair]
                for value in (float('nan'), float('inf'), -float('inf')):
                    x = clean.clone()
                    x[row, col] = value
                    xd = _on_device(x, dtype)
                    ref = _transform(kind, x[:, col:col + 1].to(dtype).float())[idx][:, 0]
                    assert not bool(torch.isfinite(ref).any()), (kind, rows, dtype, row, col, value)     # the reference: every row
                    for o, want in base.items():
                        got = _kernel(kind, xd, idx.to(DEV), o)
                        for g, w in zip(_columns_of(kind, got), _columns_of(kind, want)):
                            assert_bit_equal(g[:, others], w[:, others], f'{kind} {rows} {dtype} -> {o}: ({row}, {col}) = {value}')
                        finite = torch.ones(idx.numel(), dtype=torch.bool, device=DEV)
                        for g in _columns_of(kind, got):
                            finite &= torch.isfinite(g[:, col])
                        assert not bool(finite.any()), (kind, rows, dtype, o, row, col, value)


@pytest.mark.parametrize('kind', ('dct', 'dft'))
def test_the_padding_behind_ld_is_never_read(kind):
    """NaN, Inf and 1e30 in the columns between `features` and the leading dimension, odd feature counts: bit-identical to the call on a
    contiguous copy"""
    for rows, features, pad in ((256, 1, 1), (768, 33, 3), (1280, 65, 5), (16384, 67, 1), (1 << 17, 33, 2), (1 << 18, 7, 9)):
        g = torch.Generator().manual_seed(rows)
        x = torch.randn(rows, features, generator=g)
        idx = torch.cat([torch.tensor([0, rows // 2, rows - 1]), torch.randint(0, rows, (500, ), generator=g)]).to(DEV)
        for dtype in DTYPES:
            plain = x.to(dtype).to(DEV)
            for fill in (float('nan'), float('inf'), 1e30):
                wide = torch.full((rows, features + pad), fill).to(dtype).to(DEV)
                wide[:, :features] = plain
                view = wide[:, :features]
                assert view.stride(0) == features + pad
                for o in _out_dtypes(kind, dtype):
                    assert_bit_equal(_kernel(kind, view, idx, o), _kernel(kind, plain, idx, o), f'{kind} {rows} x {features} + {pad} {dtype} -> {o}, {fill}',
                                     nan_equal=False)


@pytest.mark.parametrize('kind', ('dct', 'dft'))
def test_out_in_the_middle_of_a_buffer_is_written_exactly(kind):
    """`out` a contiguous view in the middle of a larger buffer of a sentinel byte, prefilled with NaN: every byte before and after it
    unchanged, every entry inside written (and equal to the call that allocates its own); both DFT out dtypes"""
    for rows, features in ((1024, 37), (12288, 64), (1 << 18, 5)):
        g = torch.Generator().manual_seed(features)
        idx = torch.cat([torch.tensor([0, rows // 2, rows - 1]), torch.randint(0, rows, (700, ), generator=g)]).to(DEV)
        for dtype in DTYPES:
            x = torch.randn(rows, features, generator=g).to(dtype).to(DEV)
            for o in _out_dtypes(kind, dtype):
                shape = (idx.numel(), features) if kind == 'dct' else (2, idx.numel(), features)
                size = o.itemsize
                lead, tail = 3 * size, 4099 * size
                nbytes = math.prod(shape) * size
                buf = torch.full((lead + nbytes + tail, ), 0xa5, dtype=torch.uint8, device=DEV)
                out = buf[lead:lead + nbytes].view(o).view(shape)
                out.fill_(float('nan'))
                if kind == 'dct':
                    y = cabi.sampled_dct(x, idx, out=out)
                else:
                    y = cabi_x.sampled_dft(x, idx, out_dtype=o, out=out)
                assert y.data_ptr() == out.data_ptr()
                assert bool((buf[:lead] == 0xa5).all()) and bool((buf[lead + nbytes:] == 0xa5).all()), (kind, rows, features, dtype, o)
                assert not bool(torch.isnan(out).any()), (kind, rows, features, dtype, o)
                assert torch.equal(bits(out), bits(_kernel(kind, x, idx, o)))


@pytest.mark.parametrize('dtype', (torch.float32, torch.bfloat16))
@pytest.mark.parametrize('kind', ('dct', 'dft'))
def test_the_layer_agrees_with_torch_fft_column_by_column_when_feature_scales_differ(kind, dtype, monkeypatch):
    """linear_grp(matmul=kind) on the kernel pair and on the torch.fft formulation handed the SAME rows (the seed pinned), features scaled
    2^-8 / 1 / 2^8 by pair: every column of the weight gradient agrees to 2e-5 (fp32) or 3e-2 (bf16) of that column's largest entry"""
    seed = 0x1234567890abcdef
    monkeypatch.setattr(linear, '_draw_seed', lambda generator: seed)
    for rows in (512, 768, 1280):
        g = torch.Generator().manual_seed(rows)
        scales = torch.tensor((2.0**-8, 1.0, 2.0**8))[(torch.arange(40) // 2) % 3]
        x = (torch.randn(rows, 40, generator=g) * scales).to(dtype).to(DEV)
        w = (torch.randn(24, 40, generator=g) * 0.3).to(dtype).to(DEV)
        gy = torch.randn(rows, 24, generator=g).to(dtype).to(DEV)
        assert f'sampled_{kind}' in linear.sampled_transform_path(kind, x)
        grads = {}
        for native in (True, False):
            prev = linear.use_native_sketch(native)
            if not native:
                monkeypatch.setattr(linear, '_sampled_rows', lambda p, n, like, gen: cabi.sampled_rows(seed, n, p).to(like.device))
            try:
                wi = w.clone().requires_grad_()
                fewbit.functional.linear_grp(x, wi, None, proj_dim_ratio=0.25, matmul=kind).backward(gy)
                grads[native] = wi.grad.double()
            finally:
                linear.use_native_sketch(prev)
        rel = (grads[True] - grads[False]).abs().amax(0) / grads[False].abs().amax(0)
        print(f'\nlayer {kind} {dtype} rows {rows}: worst per-column difference {float(rel.max()):.3g}')
        assert float(rel.max()) <= (2e-5 if dtype == torch.float32 else 3e-2), (rows, rel.tolist())
