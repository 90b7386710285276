"""helpers.sampled_rows_check, the comparison of tests/test_gpu_transform_splits.py, has teeth: shown on the host, without a GPU.

The "kernel" is the float64 transform itself, rounded to fp32 or spoiled in one of the ways a wrong digit map, a wrong sign or a wrong
column index of a kernel pair would spoil it.  256 rows x 7 features of the data the GPU file uses (multiples of 1/16 below 4), every k
once in a shuffled order, a scale other than 1."""
import numpy as np
import pytest
import torch

import fewbit
from helpers import ROUNDING, TRANSFORM_EPS, sampled_rows_check

ROWS, FEATURES, SCALE = 256, 7, 0.75


def _want(kind):
    """-> (the float64 rows [idx] * SCALE: complex for 'dft'; idx)"""
    x = torch.randint(-64, 64, (ROWS, FEATURES), generator=torch.Generator().manual_seed(5)).double() / 16.0
    idx = torch.randperm(ROWS, generator=torch.Generator().manual_seed(6))
    if kind == 'dft':
        return torch.from_numpy(np.fft.fft(x.numpy(), axis=0, norm='ortho'))[idx] * SCALE, idx
    return fewbit.fft.dct(x, dim=0, norm='ortho')[idx] * SCALE, idx


def _as_result(want, dtype=torch.float32):
    """what a kernel hands back: rows of `dtype`, two planes for a complex transform"""
    return (torch.stack([want.real, want.imag]) if want.is_complex() else want).to(dtype)


@pytest.mark.parametrize('kind', ('dct', 'dft'))
def test_the_float64_rows_rounded_to_the_result_dtype_are_accepted(kind):
    want, _ = _want(kind)
    for dtype, rel in ROUNDING.items():
        ok, worst = sampled_rows_check(_as_result(want, dtype), want, rel)
        print(f'\n{kind} rounded to {dtype}: worst err / bound {worst:.3g}')
        assert ok and worst <= 1.0, (kind, dtype, worst)
    # numpy and torch references, host results of either layout
    assert sampled_rows_check(_as_result(want), want.numpy())[0]


@pytest.mark.parametrize('kind', ('dct', 'dft'))
def test_rows_k_and_n_minus_k_swapped_are_rejected(kind):
    want, idx = _want(kind)
    inverse = torch.empty_like(idx)
    inverse[idx] = torch.arange(ROWS)
    swapped = want[inverse[(ROWS - idx) % ROWS]]                     # entry j holds row N - idx[j] (row 0 stays)
    assert torch.equal(swapped[idx == 0], want[idx == 0])
    ok, worst = sampled_rows_check(_as_result(swapped), want)
    assert not ok and worst > 1e3, (kind, worst)


def test_an_imaginary_plane_of_the_wrong_sign_is_rejected():
    want, _ = _want('dft')
    ok, worst = sampled_rows_check(_as_result(want.conj()), want)
    assert not ok and worst > 1e3, worst
    # the real plane alone is fine: the rejection is the imaginary plane's
    assert sampled_rows_check(_as_result(want)[0], want.real)[0]


@pytest.mark.parametrize('kind', ('dct', 'dft'))
def test_one_column_shifted_by_one_feature_is_rejected(kind):
    want, _ = _want(kind)
    got = _as_result(want)
    got[..., 3] = got[..., 4].clone()                                # column 3 holds column 4's values; every other column is right
    ok, worst = sampled_rows_check(got, want)
    assert not ok and worst > 1e3, (kind, worst)


@pytest.mark.parametrize('kind', ('dct', 'dft'))
def test_an_error_of_twice_the_bound_in_a_single_entry_is_rejected_and_half_the_bound_accepted(kind):
    want, _ = _want(kind)
    planes = torch.stack([want.real, want.imag]) if want.is_complex() else want
    top = float(planes.abs().max())
    for dtype, rel in ROUNDING.items():
        at = (-1, 17, 5)[3 - planes.dim():]                           # one entry (of the imaginary plane for 'dft')
        bound = rel * abs(float(planes[at])) + TRANSFORM_EPS * top
        for factor, verdict in ((2.0, False), (0.5, True)):
            got = planes.clone()                                     # float64: only the planted error is there
            got[at] += factor * bound
            ok, worst = sampled_rows_check(got, want, rel)
            assert ok is verdict and abs(worst - factor) < 1e-6, (kind, dtype, factor, worst)


def test_a_result_of_another_shape_or_with_a_non_finite_entry_is_rejected():
    want, _ = _want('dct')
    assert not sampled_rows_check(_as_result(want)[:-1], want)[0]
    got = _as_result(want)
    got[3, 2] = float('nan')
    assert not sampled_rows_check(got, want)[0]
    got[3, 2] = float('inf')
    assert not sampled_rows_check(got, want)[0]
