"""The row counts 7 x 2^k (3584 .. 57344), 9 x 2^k (2304 .. 36864) and 15 x 2^k (3840 .. 30720) of the sampled transforms, without a GPU:
both libraries answer their workspace query with the one formula, the layer's row predicate follows, the neighbours and the counts just
outside each family are refused with a text that names the families, and the rows of a seed are the documented 32-bit-word rule."""
import pytest
import torch

import sketch_reference as ref
from fewbit_amd import cabi, cabi_x, linear

FAMILIES = {7: range(9, 14), 9: range(8, 13), 15: range(8, 12)}
NEW_ROWS = [m << k for m, ks in FAMILIES.items() for k in ks]
# just outside each family, other odd factors, and the count the existing tests pin
REFUSED = [1792, 7 << 14, 9 << 7, 9 << 13, 15 << 7, 15 << 12, 11 << 9, 13 << 9]
NAMES = ('7 x 2^k (3584 .. 57344)', '9 x 2^k (2304 .. 36864)', '15 x 2^k (3840 .. 30720)')


def test_the_new_row_counts_are_the_ones_of_the_issue():
    assert sorted(NEW_ROWS) == sorted([3584, 7168, 14336, 28672, 57344, 2304, 4608, 9216, 18432, 36864, 3840, 7680, 15360, 30720])


@pytest.mark.parametrize('dtype', (torch.float32, torch.float16, torch.bfloat16))
def test_both_libraries_give_the_workspace_formula_at_every_new_row_count(dtype):
    for rows in NEW_ROWS:
        for features, proj in ((1, 1), (64, 10), (770, 3276), (3072, rows // 5)):
            want = -(-features // 64) * rows * 256 + 2048 + -(-8 * proj // 16) * 16
            assert cabi.sampled_dct_workspace_bytes(rows, features, proj, dtype) == want, (rows, features, proj)
            assert cabi_x.sampled_dft_workspace_bytes(rows, features, proj, dtype) == want, (rows, features, proj)
        assert linear._transform_rows('dct', rows) and linear._transform_rows('dft', rows), rows


def test_neighbours_and_counts_outside_the_families_are_refused_and_the_text_names_the_families():
    L = cabi_x.lib()
    for rows in sorted({r + d for r in NEW_ROWS for d in (-1, 1)} | set(REFUSED)):
        assert cabi.sampled_dct_workspace_bytes(rows, 64, 10) == 0 == cabi_x.sampled_dft_workspace_bytes(rows, 64, 10), rows
        assert not linear._transform_rows('dct', rows) and not linear._transform_rows('dft', rows), rows
        with pytest.raises(cabi.FewbitHipError) as e:
            cabi.sampled_rows(1, rows, 4)
        assert f'rows = {rows}' in str(e.value) and all(name in str(e.value) for name in NAMES), str(e.value)
        assert L.fewbit_hipx_sampled_dft_seeded(0, None, rows, 8, 8, 1, None, 4, 1.0, 0, None, None, 0, None) == -2
        text = L.fewbit_hipx_last_error().decode()
        assert f'rows = {rows}' in text and all(name in text for name in NAMES), text
    assert all(name.replace(' .. ', ', ').replace('(', 'in [').replace(')', ']') in cabi.SAMPLED_ROWS for name in NAMES)


@pytest.mark.parametrize('rows', (7 << 9, 9 << 9, 15 << 8))
def test_rows_of_a_seed_are_the_32_bit_word_rule(rows):
    """idx[j] = (word j % 4 of Philox4x32-10((j / 4, 0, 0, 3), seed) x rows) >> 32 (include/fewbit_hip.h), against the independent Philox of
    tests/sketch_reference.py"""
    seed = 0x0123456789abcdef
    key = (seed & 0xffffffff, seed >> 32)
    idx = cabi.sampled_rows(seed, rows, 1003)
    want = [(int(w) * rows) >> 32 for q in range(251) for w in ref.philox4x32(q, 0, 0, 3, *key)][:1003]
    assert idx.tolist() == want and 0 <= min(want) and max(want) < rows


def test_every_sampled_row_is_below_the_row_count():
    for n, rows in enumerate(NEW_ROWS):
        idx = cabi.sampled_rows(0x9e3779b97f4a7c15 * (n + 1) & 0xffffffffffffffff, rows, 100003)
        assert idx.dtype == torch.int64 and 0 <= int(idx.min()) and int(idx.max()) < rows, rows


def test_the_rows_of_a_seed_are_uniform_over_3584_bins():
    """chi-square of 3584 x 1024 samples over the 3584 bins against the 99.99 % point of 3583 degrees of freedom"""
    from scipy.stats import chi2
    rows, mean = 7 << 9, 1024
    counts = torch.bincount(cabi.sampled_rows(7, rows, rows * mean), minlength=rows).double()
    assert counts.numel() == rows
    stat = float(((counts - mean) ** 2 / mean).sum())
    bound = float(chi2.ppf(0.9999, rows - 1))
    print(f'\nchi-square over {rows} bins: {stat:.1f}, 99.99 % point of {rows - 1} degrees of freedom: {bound:.1f}')
    assert stat < bound, (stat, bound)
