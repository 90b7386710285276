"""The per-column criterion of tests/test_gpu_transform_columns.py has teeth: shown on the host, without a GPU, on a model of the kernels.

The model is the sampled DFT pair's arithmetic in complex64 (torch.fft on the host): features (2c, 2c + 1) packed as one complex column,
the four-step split N = N1 x N2 = 128 x 128 (length-N1 transforms over rows N2 apart, the twiddle W_N^{n2 k1}, length-N2 transforms),
the split of Z[k], conj Z[N - k] back into the two columns and the factor 1 / sqrt(N).  The fp32 reference is torch.fft in complex64 with
every column apart; the exact one is the float64 transform of the same (rounded) input.

    the correct model          passes the per-column criterion on every structured family, and the per-pair one on partners 2^20 apart
    the correct model          fails the per-column criterion on partners 2^20 apart (the pair coupling: what the test records, not bounds)
    a bf16 intermediate        (the variant rejected in round 6: A[k1][n2] rounded to bf16 between the passes) fails it on white noise,
                               a mean of 1000 sigma and a random walk
"""
import math

import pytest
import torch

from helpers import (TRANSFORM_FAMILIES, normalised_error, reference_error, transform_error_check, transform_input, transform_rows)

ROWS, N1, FEATURES = 16384, 128, 13


def packed_four_step(x: torch.Tensor, bf16_intermediate: bool = False) -> torch.Tensor:
    """the complex64 (rows, features) DFT (norm='ortho') of the float32 matrix x as the kernel pair computes it"""
    rows, features = x.shape
    n2 = rows // N1
    if features % 2:
        x = torch.cat([x, torch.zeros(rows, 1, dtype=x.dtype)], 1)           # the partnerless last column: a zero partner
    z = torch.complex(x[:, 0::2], x[:, 1::2])                                 # row n = N2 n1 + b
    a = torch.fft.fft(z.reshape(N1, n2, -1), dim=0)                           # [k1][n2]
    k1 = torch.arange(N1, dtype=torch.float64)[:, None]
    b = torch.arange(n2, dtype=torch.float64)[None, :]
    tw = torch.polar(torch.ones(N1, n2, dtype=torch.float64), -2 * math.pi * ((k1 * b) % rows) / rows).to(torch.complex64)
    a = a * tw[:, :, None]
    if bf16_intermediate:
        a = torch.complex(a.real.bfloat16().float(), a.imag.bfloat16().float())
    zk = torch.fft.fft(a, dim=1).transpose(0, 1).reshape(rows, -1)           # Z[k1 + N1 k2]
    zm = zk[(-torch.arange(rows)) % rows].conj()                             # conj Z[N - k]
    factor = torch.tensor(1.0 / math.sqrt(rows), dtype=torch.float32)
    even, odd = (zk + zm) * 0.5 * factor, (zk - zm) * (-0.5j) * factor
    out = torch.stack([even, odd], 2).reshape(rows, -1)
    return out[:, :features]


def _case(family, bf16_intermediate=False, pair=False):
    x, k0 = transform_input(family, 'dft', ROWS, FEATURES, torch.float32, 11)
    idx = transform_rows(ROWS, k0, 1000, 12)
    want = torch.fft.fft(x, dim=0, norm='ortho')[idx]
    ref32 = torch.fft.fft(x.float(), dim=0, norm='ortho')[idx]
    got = packed_four_step(x.float(), bf16_intermediate)[idx]
    e_ref = reference_error(ref32, want, x, pair)
    ok, worst, ratio = transform_error_check(got, want, x, e_ref, 0.0, pair)
    print(f'\nmodel {family:16s} bf16 intermediate {bf16_intermediate!s:5s} {"per pair  " if pair else "per column"}: '
          f'E_ref / (u log2 N) {e_ref / (2.0**-24 * math.log2(ROWS)):6.2f}, kernel / max(E_ref, u log2 N) {ratio:10.3g}, worst err / bound {worst:10.3g}')
    return ok, got, x


def test_the_model_is_the_dft():
    """(the model itself: within fp32 rounding of the float64 transform, every column)"""
    x, _ = transform_input('white noise', 'dft', ROWS, FEATURES, torch.float32, 3)
    err = normalised_error(packed_four_step(x.float()), torch.fft.fft(x, dim=0, norm='ortho'), x)
    assert float(err.max()) < 1e-5


@pytest.mark.parametrize('family', TRANSFORM_FAMILIES)
def test_the_correct_packed_four_step_passes_every_family(family):
    ok, _, _ = _case(family)
    assert ok, family


def test_the_correct_packed_four_step_passes_the_pair_criterion_and_keeps_a_zero_pair_exact():
    ok, got, x = _case('partners', pair=True)
    assert ok
    assert bool((got[:, 2:4] == 0).all())                                    # by value: -0 counts
    assert float(x[:, 2:4].abs().max()) == 0.0 and float(x[:, :2].abs().max()) > 0.0


def test_the_correct_packed_four_step_fails_the_per_column_bound_on_partners_2_20_apart():
    ok, _, _ = _case('partners')
    assert not ok


@pytest.mark.parametrize('family', TRANSFORM_FAMILIES[:3])
def test_a_bf16_intermediate_fails_the_per_column_bound(family):
    ok, _, _ = _case(family, bf16_intermediate=True)
    assert not ok, family
