"""The tile body and the element-wise tail of every streaming activation kernel give the same bytes.

Whole tiles go through the vectorised body of a kernel (GroupIO load / store), whatever does not fill a tile through the element-wise tail of the
last wave (Elem load / store): separate code, separate conversions, separately compiled -- and how many elements of a tensor sit in the tail
(n mod 512 U) changes with U and with the launch policy, so a difference between the two breaks "the same bytes at every launch shape".  Every case
puts the SAME inputs through both (helpers.run_body: one call of 65 x 1024 elements, no tail at U = 1 and at U = 2; helpers.run_tail: calls of at
most 511 elements, no tile), with the groups per lane forced to 1 and to 2, and asserts that all four runs agree bit for bit in the values (NaN by
position) and in the unpacked codes.  Inputs: every pattern of the 16-bit dtypes, helpers.probe_patterns for fp32.

Seen on the MI355X before Elem<FEWBIT_F16>::store got its register barrier (the fp16 tails ended in v_fma_mixlo_f16: the exact product rounded once, +0
added; the bodies round to fp32 and convert): of the 65 536 fp16 inputs the value differed at 9867 for silu, 9871 for mish (mostly -0 in a tile, +0 in the tail),
2 for gelu, 2 for elu 0.7, 20 / 103 / 63 for leaky_relu 0.01 / 0.1 / 0.3 -- the same count in all four forward families and at both U; celu, softplus and
everything in bf16 and fp32 agreed (EXPERIMENTS.md section 8.14)."""
import pytest
import torch

import step1_reference
from fewbit_amd import cabi
from fewbit_amd.store import store
from helpers import BODY_N, GEOMETRIES, STEP1_CASES, STREAM_TUNE_KEYS, TAIL_N, case_id, differing, kinks, probe_patterns, run_geometry, set_groups_per_lane

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DTYPES = (torch.float32, torch.float16, torch.bfloat16)

# the parameters of tests/test_gpu_numerics.py
CONTINUOUS = [('celu', (1.3, )), ('elu', (0.7, )), ('gelu', ()), ('hardswish', ()), ('logsigmoid', ()), ('mish', ()), ('selu', ()), ('sigmoid', ()),
              ('silu', ()), ('softplus', (2.0, 5.0)), ('softplus', (1.0, 20.0)), ('softsign', ()), ('tanh', ()), ('tanhshrink', ()), ('identity', ()),
              ('identity_fold', (0.375, ))]
# the forward families: (tuning, levels of the table, the kernel the call must take)
FAMILIES = {'register search': ({}, 8, 'quantize_forward_kernel<'), 'pattern table': ({'lut_min': 0}, 8, 'quantize_forward_lut_kernel<'),
            'LDS search': ({}, 40, 'quantize_forward_wide_kernel<'), 'wide pattern table': ({'lut_min': 0}, 40, 'quantize_forward_lut_wide_kernel<')}


@pytest.fixture(autouse=True)
def _restore_launch_policy():
    yield
    cabi.tune(**{k: -1 for k in STREAM_TUNE_KEYS})


def call_sizes(n):
    """the distinct element counts of the calls of one case"""
    return sorted({BODY_N, TAIL_N, n % TAIL_N or TAIL_N})


def borders_of(name, nlevels, dtype):
    """inner borders: the built-in 3-bit table where there is one, else (identity, folded identity, 40 levels) an even grid rounded to the dtype"""
    if nlevels == 8 and (name, 3) in store:
        return store.get(name, 3, 'cpu', dtype)[0][1:-1].contiguous()
    b = torch.unique(torch.linspace(0.05 if name == 'identity_fold' else -3.0, 3.0, nlevels - 1).to(dtype))
    assert b.numel() == nlevels - 1
    return b


def compare(runs, what, problems):
    """every run against the first, output by output; a difference is printed with its count and the first inputs, and kept for the assertion"""
    (first, base), *others = runs
    for label, outs in others:
        for which, a, b in zip(('values', 'codes', 'gradients'), base, outs):
            d = differing(a, b)
            if bool(d.any()):
                idx = d.nonzero().flatten()[:4].tolist()
                problems.append(f'{what}: {which} of {label} differ from {first} at {int(d.sum())} inputs, first at {idx}: {first} {a[idx].tolist()}, {label} {b[idx].tolist()}')
                print(problems[-1])


@pytest.mark.parametrize('dtype', DTYPES, ids=str)
@pytest.mark.parametrize('name,p', CONTINUOUS, ids=case_id)
def test_forward_tail_is_body(name, p, dtype):
    x = probe_patterns(dtype, kinks(p))
    problems = []
    for family, (tuning, nlevels, kernel) in FAMILIES.items():
        if 'lut_min' in tuning and (dtype == torch.float32 or name == 'identity_fold'):
            continue                                    # the pattern table exists for 16-bit inputs searched by their own value
        borders = borders_of(name, nlevels, dtype).to(DEV)
        k = cabi.bitwidth(nlevels)
        cabi.tune(lut_min=tuning.get('lut_min', -1))

        def op(xs):
            y, state = cabi.quantize_forward(name, xs, borders, *p)
            return y, cabi.unpack_codes(state, xs.numel(), k)
        runs = []
        for where, u in GEOMETRIES:
            set_groups_per_lane(u)
            for n in call_sizes(x.numel()):            # a policy change must not turn the families into runs of one kernel
                assert cabi.describe_forward(name, dtype, n, nlevels - 1)['kernel'].startswith(kernel), (family, n, cabi.describe_forward(name, dtype, n, nlevels - 1))
            runs.append((f'{where} U={u}', run_geometry(where, op, x)))
        compare(runs, f'{name}{p} {dtype} {family}', problems)
    assert not problems, '\n'.join(problems)


@pytest.mark.parametrize('dtype', DTYPES, ids=str)
@pytest.mark.parametrize('name,p', STEP1_CASES, ids=case_id)
def test_stepwise1_tail_is_body(name, p, dtype):
    x = probe_patterns(dtype, kinks(p))
    gy = torch.roll(x, 12345)
    problems = []

    def op(xs, gs):
        y, state = cabi.stepwise1_forward(name, xs, *p)
        return y, cabi.unpack_codes(state, xs.numel(), 1), cabi.stepwise1_backward(name, gs, state, *p[:1])
    runs = []
    for where, u in GEOMETRIES:
        set_groups_per_lane(u)
        for n in call_sizes(x.numel()):
            for plan in (cabi.describe_stepwise1_forward(name, dtype, n), cabi.describe_stepwise1_backward(name, dtype, n)):
                assert plan['kernel'].startswith('stepwise1_') and plan['u'] == u, plan
        runs.append((f'{where} U={u}', run_geometry(where, op, x, gy)))
    compare(runs, f'{name}{p} {dtype}', problems)
    assert not problems, '\n'.join(problems)


def levels_of(nlevels, dtype, variant):
    """levels with 0.0, a negative value, 0.3 and -1.7 among them (two levels hold two of the four: `variant` picks which), the rest seeded, rounded to the dtype"""
    fixed = [0.0, -1.7, 0.3, -0.0625]
    if nlevels < 4:
        fixed = fixed[2 * variant:2 * variant + 2]
    rest = torch.rand(max(nlevels - len(fixed), 0), generator=torch.Generator().manual_seed(nlevels)) * 4 - 2
    return torch.cat([torch.tensor(fixed), rest])[:nlevels].to(dtype)


@pytest.mark.parametrize('dtype', DTYPES, ids=str)
@pytest.mark.parametrize('nlevels', (2, 4, 8, 16, 40))
def test_backward_tail_is_body_is_host_product(nlevels, dtype):
    """gx = levels[code] * gy for every gy pattern against every level of a small table (codes (i + r) mod nlevels): body == tail, and both equal the
    fp32 product rounded once to the dtype, computed on the host -- a zero level times a negative gy stays -0"""
    gy = probe_patterns(dtype, kinks(()))
    k = cabi.bitwidth(nlevels)
    kernel = 'quantize_backward_kernel<' if k <= 4 else 'quantize_backward_wide_kernel<'
    problems = []
    for variant in range(2 if nlevels < 4 else 1):
        levels = levels_of(nlevels, dtype, variant)
        dev_levels = levels.to(DEV)
        for r in range(min(nlevels, 4)):
            codes = ((torch.arange(gy.numel()) + r) % nlevels).to(torch.int32)
            want = (levels.float()[codes.long()] * gy.float()).to(dtype)

            def op(gs, cs):
                return (cabi.quantize_backward(gs, cabi.pack_codes(cs.contiguous(), k), dev_levels), )
            runs = [('host product', (want, ))]
            for where, u in GEOMETRIES:
                set_groups_per_lane(u)
                for n in call_sizes(gy.numel()):
                    plan = cabi.describe_backward(dtype, n, nlevels)
                    assert plan['kernel'].startswith(kernel) and plan['bits'] == k and (k > 4 or plan['u'] == u), plan
                runs.append((f'{where} U={u}', run_geometry(where, op, gy, codes)))
            compare(runs, f'{nlevels} levels {levels[:4].tolist()} rotation {r} {dtype}', problems)
    assert not problems, '\n'.join(problems)


def test_stepwise1_backward_is_host_product():
    """the 1-bit backward against step1_reference.backward on a zero multiplier and a negative gy: -0, in the body and in the tail, every dtype"""
    for dtype in DTYPES:
        gy = probe_patterns(dtype)
        bit = (torch.arange(gy.numel()) % 3) == 0
        want = step1_reference.backward('relu', gy, bit)
        codes = bit.to(torch.int32)

        def op(gs, cs):
            return (cabi.stepwise1_backward('relu', gs, cabi.pack_codes(cs.contiguous(), 1)), )
        problems = []
        runs = [('host product', (want, ))]
        for where, u in GEOMETRIES:
            set_groups_per_lane(u)
            runs.append((f'{where} U={u}', run_geometry(where, op, gy, codes)))
        compare(runs, f'relu backward {dtype}', problems)
        assert not problems, '\n'.join(problems)
        neg = (gy.float() < 0) & ~bit
        assert bool(torch.signbit(runs[1][1][0][neg]).all())
