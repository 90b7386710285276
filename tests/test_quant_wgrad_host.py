"""The weight gradient from the packed form without a GPU (include/fewbit_hipx.h, fewbit_hipx_quant_wgrad; fewbit_amd/csrc/fewbit_qgemm.hip): the two
entry points (declared, exported, bound), the plan and its workspace cap, and what is refused before anything is launched."""
import itertools
import re
import subprocess
from pathlib import Path

import pytest
import torch

from fewbit_amd import cabi_x, linear

ROOT = Path(__file__).resolve().parents[1]
G, P, O, W = 0x10000, 0x20000, 0x30000, 0x40000                   # addresses that are never dereferenced
F32, F16, BF16 = 0, 1, 2


def test_the_symbols_are_declared_exported_and_bound_and_the_revision_is_still_2():
    header = (ROOT / 'include' / 'fewbit_hipx.h').read_text()
    out = subprocess.run(['nm', '-D', '--defined-only', str(cabi_x.LIB_PATH)], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in ('fewbit_hipx_quant_wgrad_workspace', 'fewbit_hipx_quant_wgrad'):
        assert re.search(name + r'\s*\(', header) and name in exported and name in cabi_x.SYMBOLS
    assert cabi_x.lib().fewbit_hipx_revision() == cabi_x.REVISION == 2 and re.search(r'#define FEWBIT_HIPX_REVISION 2\b', header)
    assert {'quant_wgrad', 'quant_wgrad_workspace', 'quant_wgrad_serves', 'quant_wgrad_slices', 'QUANT_WGRAD_TILE'} <= set(cabi_x.__all__)
    assert linear.use_fused_weight_gradient() is False and 'use_fused_weight_gradient' in linear.__all__        # off by default


def test_the_predicate_the_plan_and_the_workspace_query_agree():
    bm, bn, bk = cabi_x.QUANT_WGRAD_TILE
    for dtype, bits, fin, fout, rows in itertools.product((torch.float32, torch.float16, torch.bfloat16), (1, 2, 3, 4, 8, 16), (0, 8, 64, 72, 128, bn + 64),
                                                          (0, 4, 8, 12, bm - 8, bm + 8), (0, 1, bk + 9, 5000)):
        serves = cabi_x.quant_wgrad_serves(dtype, rows, fin, fout, bits)
        assert serves == (dtype != torch.float32 and bits in (2, 4, 8) and rows > 0 and fin > 0 and fin % 64 == 0 and fout > 0 and fout % 8 == 0)
        slices = cabi_x.quant_wgrad_slices(rows, fin, fout) if serves else 1
        assert cabi_x.quant_wgrad_workspace(dtype, rows, fin, fout, bits) == (4 * slices * fout * fin if slices > 1 else 0), (dtype, bits, fin, fout, rows)
    assert cabi_x.lib().fewbit_hipx_quant_wgrad_workspace(7, 5000, 64, 8, 4) == 0


@pytest.mark.parametrize('rows, fin, fout', ((16384, 768, 3072), (16384, 3072, 768), (16384, 4096, 11008), (1, 768, 3072), (1, 64, 8), (200, 64, 8)))
def test_the_workspace_stays_within_the_decoded_tensor_it_replaces(rows, fin, fout):
    bm, bn, bk = cabi_x.QUANT_WGRAD_TILE
    slices = cabi_x.quant_wgrad_slices(rows, fin, fout)
    need = cabi_x.quant_wgrad_workspace(torch.bfloat16, rows, fin, fout, 4)
    assert need == (4 * slices * fout * fin if slices > 1 else 0) and need <= rows * fin * 2
    assert 1 <= slices <= -(-rows // bk) and slices * -(-fin // bn) * -(-fout // bm) <= max(256, -(-fin // bn) * -(-fout // bm))
    assert slices == {(16384, 768, 3072): 2, (16384, 3072, 768): 3, (200, 64, 8): 4}.get((rows, fin, fout), 1)


def test_every_refusal_names_the_call_before_anything_is_launched():
    call = cabi_x.lib().fewbit_hipx_quant_wgrad
    size = cabi_x.quant_bytes(5000 * 64, 4)
    need = cabi_x.quant_wgrad_workspace(torch.bfloat16, 5000, 64, 8, 4)
    assert need > 0

    def refused(rc, code, *words):
        message = cabi_x.lib().fewbit_hipx_last_error().decode()
        assert rc == code and all(word in message for word in ('quant_wgrad', ) + words), (rc, message)

    ok = dict(dtype=BF16, grad=G, ld=8, packed=P, size=size, rows=5000, fin=64, fout=8, bits=4, out_dtype=F32, out=O, ws=W, ws_bytes=need)

    def go(**change):
        a = {**ok, **change}
        return call(a['dtype'], a['grad'], a['ld'], a['packed'], a['size'], a['rows'], a['fin'], a['fout'], a['bits'], a['out_dtype'], a['out'], a['ws'], a['ws_bytes'], None)

    refused(go(dtype=7), -1, 'unknown dtype 7')
    refused(go(out_dtype=9), -1, 'unknown dtype 9')
    refused(go(bits=3), -2, 'bits = 3')
    refused(go(dtype=F32), -2, 'fp32 gradients')
    refused(go(out_dtype=F16), -1, 'out_dtype')
    refused(go(rows=0), -1, 'rows = 0')
    refused(go(fin=72), -2, 'in_features = 72')
    refused(go(fout=12, ld=16), -2, 'out_features = 12')
    refused(go(ld=4), -1, 'ld_grad = 4')
    refused(go(fout=16, ld=8), -1, 'ld_grad = 8')
    for name in ('grad', 'packed', 'out', 'ws'):
        refused(go(**{name: None}), -1, 'null pointer')
    refused(go(grad=G + 8), -1, 'grad must be 16-byte aligned')
    refused(go(packed=P + 4), -1, 'packed must be 8-byte aligned')
    refused(go(out=O + 8), -1, 'out must be 16-byte aligned')
    refused(go(ws=W + 8), -1, 'the workspace must be 16-byte aligned')
    refused(go(size=size - 1), -1, f'packed has {size - 1} bytes, {size} are needed')
    refused(go(ws_bytes=need - 1), -1, f'the workspace has {need - 1} bytes, {need} are needed')
