"""The LM head and its loss as one node, without a GPU (fewbit_amd/xent.py, linear_cross_entropy; include/fewbit_hipx.h, fewbit_hipx_cross_entropy_step):
the entry point of the step (declared, exported, bound), what it refuses before anything is launched, the default chunk, and the layer off the kernel
path, where it is ``F.cross_entropy(F.linear(...))`` bit for bit."""
import re
import subprocess
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

import fewbit
from fewbit_amd import cabi_x, xent

ROOT = Path(__file__).resolve().parents[1]
P, T, G, L, S = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000        # addresses that are never dereferenced
BF16 = 2


def test_the_symbol_is_declared_exported_and_bound_and_the_revision_is_still_2():
    header = (ROOT / 'include' / 'fewbit_hipx.h').read_text()
    out = subprocess.run(['nm', '-D', '--defined-only', str(cabi_x.LIB_PATH)], check=True, capture_output=True, text=True).stdout
    name = 'fewbit_hipx_cross_entropy_step'
    assert re.search(name + r'\s*\(', header) and name in {line.split()[-1] for line in out.splitlines() if line.strip()} and name in cabi_x.SYMBOLS
    assert cabi_x.lib().fewbit_hipx_revision() == cabi_x.REVISION == 2 and re.search(r'#define FEWBIT_HIPX_REVISION 2\b', header)
    assert {'cross_entropy_step', 'CROSS_ENTROPY_STEP_STAGED_BYTES'} <= set(cabi_x.__all__)
    assert fewbit.functional.linear_cross_entropy is xent.linear_cross_entropy is fewbit.linear_cross_entropy
    assert fewbit.LinearCrossEntropyLoss is xent.LinearCrossEntropyLoss


def test_the_step_refuses_by_name_before_anything_is_launched():
    step = cabi_x.lib().fewbit_hipx_cross_entropy_step

    def refused(rc, *words):
        message = cabi_x.lib().fewbit_hipx_last_error().decode()
        assert rc < 0 and all(word in message for word in ('cross_entropy_step', ) + words), (rc, message)

    refused(step(7, P, 3, 8, 8, T, -100, G, 0, L, S, None), 'unknown dtype 7')
    refused(step(BF16, P, 0, 8, 8, T, -100, G, 0, L, S, None), 'rows = 0')
    refused(step(BF16, P, 3, 0, 8, T, -100, G, 0, L, S, None), 'width = 0')
    refused(step(BF16, P, 3, 2**24 + 1, 2**24 + 1, T, -100, G, 0, L, S, None), 'width = 16777217')
    refused(step(BF16, P, 3, 8, 7, T, -100, G, 0, L, S, None), 'ld = 7 < width = 8')
    refused(step(BF16, P, 3, 8, 8, T, -100, G, 2, L, S, None), 'grow_stride = 2')
    refused(step(BF16, None, 3, 8, 7, T, -100, G, 2, L, S, None), 'ld = 7 < width = 8')          # (the order of the launches: shape, stride, pointers)
    for x, t, grow, lse, loss in ((None, T, G, L, S), (P, None, G, L, S), (P, T, None, L, S), (P, T, G, None, S), (P, T, G, L, None)):
        refused(step(BF16, x, 3, 8, 8, t, -100, grow, 1, lse, loss, None), 'null pointer')


@pytest.mark.parametrize('rows, hidden, classes, want', ((16384, 4096, 32000, 4096), (16384, 4096, 128256, 4096), (16384, 768, 50265, 4096),
                                                         (100, 64, 1000, 100), (1, 8, 11, 1), (65536, 8192, 32000, 32768), (3000, 4096, 4096, 3000),
                                                         (4096, 4096, 4097, 4096), (8192, 4096, 8191, 8192)))
def test_the_default_chunk_is_a_power_of_two_of_about_the_hidden_states_between_4096_and_the_rows(rows, hidden, classes, want):
    assert xent.default_chunk_rows(rows, hidden, classes) == want


def same(ours, theirs, x, w, b):
    """the value and the three gradients of ``ours`` are those of ``theirs`` to the bit"""
    grads = []
    for f in (ours, theirs):
        leaves = [v.clone().requires_grad_() for v in (x, w, b)]
        y = f(*leaves)
        y.backward(torch.ones_like(y) * 0.75)
        grads.append((y.detach(), *(v.grad for v in leaves)))
    for a, c in zip(*grads):
        assert a.dtype == c.dtype and a.shape == c.shape and torch.equal(a, c)


@pytest.mark.parametrize('reduction', ('mean', 'sum', 'none'))
@pytest.mark.parametrize('dtype', (torch.float32, torch.float64, torch.bfloat16))
def test_host_tensors_and_reduction_none_are_torchs(dtype, reduction):
    g = torch.Generator().manual_seed(5)
    x, w, b = (torch.randn(shape, generator=g).to(dtype) for shape in ((7, 12), (19, 12), (19, )))
    t = torch.randint(0, 19, (7, ), generator=g)
    t[2] = -100
    want = lambda x, w, b: F.cross_entropy(F.linear(x, w, b), t, reduction=reduction)
    same(lambda x, w, b: fewbit.functional.linear_cross_entropy(x, w, t, b, reduction=reduction, chunk_rows=2, accumulate_dtype=torch.float32), want, x, w, b)
    same(lambda x, w, b: fewbit.LinearCrossEntropyLoss(reduction=reduction)(x, w, t, b), want, x, w, b)
    with pytest.raises(ValueError):
        fewbit.functional.linear_cross_entropy(x, w, t, b, reduction='median')
