"""The Python side of the sampled-transform bindings, pinned from outside: what each wrapper hands its C function (recorded in place of the
call, compared with a tuple built here from the parameter order of include/fewbit_hip.h and include/fewbit_hipx.h), what it refuses and in
which words, and what an empty call does.  Shapes are the smallest at which the paths differ: 256 rows (the smallest kernel), 768 (an odd
family), 300 rows zero-extended to 512; 70 features (one full 64-feature tile and an edge tile) in a 72-wide buffer, p = 5; fp32 and bf16.
Nothing here launches a kernel except the empty calls, which C answers before it looks at the rows."""
import pytest
import torch

from fewbit_amd import cabi, cabi_x
from fewbit_amd.cabi import FewbitHipError

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CODE = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}        # enum fewbit_dtype
FEATURES, LD, P = 70, 72, 5
ROWS = ('2^k in [256, 262144], 3 x 2^k in [768, 49152], 5 x 2^k in [1280, 40960], 7 x 2^k in [3584, 57344], 9 x 2^k in [2304, 36864] '
        'or 15 x 2^k in [3840, 30720]')
MASK = 0xffffffffffffffff

# name -> (module, C symbol, transform, zero-extended, rows come from a seed)
WRAPPERS = {
    'sampled_dct': (cabi, 'fewbit_hip_sampled_dct', 'dct', False, False),
    'sampled_dct_seeded': (cabi, 'fewbit_hip_sampled_dct_seeded', 'dct', False, True),
    'sampled_dft': (cabi_x, 'fewbit_hipx_sampled_dft', 'dft', False, False),
    'sampled_dft_seeded': (cabi_x, 'fewbit_hipx_sampled_dft_seeded', 'dft', False, True),
    'sampled_dct_zext': (cabi_x, 'fewbit_hipx_sampled_dct_zext', 'dct', True, False),
    'sampled_dct_zext_seeded': (cabi_x, 'fewbit_hipx_sampled_dct_zext_seeded', 'dct', True, True),
    'sampled_dft_zext': (cabi_x, 'fewbit_hipx_sampled_dft_zext', 'dft', True, False),
    'sampled_dft_zext_seeded': (cabi_x, 'fewbit_hipx_sampled_dft_zext_seeded', 'dft', True, True),
}
IDX_WRAPPERS = tuple(n for n, w in WRAPPERS.items() if not w[4])
SEEDED_WRAPPERS = tuple(n for n, w in WRAPPERS.items() if w[4])
DFT_WRAPPERS = tuple(n for n, w in WRAPPERS.items() if w[2] == 'dft')
PLAIN_WRAPPERS = tuple(n for n, w in WRAPPERS.items() if not w[3])
ZEXT_WRAPPERS = tuple(n for n, w in WRAPPERS.items() if w[3])


def _matrix(rows, dtype=torch.float32):
    """a rows x 70 view of a rows x 72 buffer (leading dimension 72)"""
    return torch.zeros(rows, LD, dtype=dtype, device=DEV)[:, :FEATURES]


def _idx(p=P):
    return torch.arange(p, dtype=torch.int64, device=DEV)


def _call(name, m, rows_arg, length=512, **kw):
    """the wrapper `name` on `m`; rows_arg: the idx tensor, or (p, seed); length: the transform length of a zero-extended wrapper"""
    module, _, _, zext, seeded = WRAPPERS[name]
    args = ((length, ) if zext else ()) + (tuple(rows_arg) if seeded else (rows_arg, ))
    return getattr(module, name)(m, *args, **kw)


def _rows_arg(name, p=P, seed=7):
    return (p, seed) if WRAPPERS[name][4] else _idx(p)


def _record(monkeypatch, library, symbol):
    """replace the C function on the loaded library object by a recorder that returns 0 (FEWBIT_OK): nothing is launched"""
    calls = []
    monkeypatch.setattr(library, symbol, lambda *args: (calls.append(args), 0)[1])
    return calls


def _message(call):
    with pytest.raises(FewbitHipError) as e:
        call()
    return str(e.value)


@pytest.mark.parametrize('seed_kind', ('int', 'word'))
@pytest.mark.parametrize('dtype', (torch.float32, torch.bfloat16), ids=('fp32', 'bf16'))
@pytest.mark.parametrize('name', tuple(WRAPPERS))
def test_the_arguments_handed_to_c(name, dtype, seed_kind, monkeypatch):
    """(dtype, m, rows[, valid_rows], features, ld, idx | seed, seed_device, proj, scale[, out_dtype], out, workspace, workspace_bytes, stream);
    'int': given out / workspace / stream and an int seed beyond 64 bits; 'word': everything allocated by the wrapper, torch's current stream
    and a device seed word.  The wrappers that take idx run both ways with the same idx."""
    module, symbol, kind, zext, seeded = WRAPPERS[name]
    side = torch.cuda.Stream(DEV)
    word = torch.tensor([77], dtype=torch.int64, device=DEV)
    idx = _idx()
    for rows in ((300, ) if zext else (256, 768)):
        m = _matrix(rows, dtype)
        length = 512 if zext else rows
        lead = (512, 300) if zext else (rows, )
        query = cabi.sampled_dct_workspace_bytes if name in ('sampled_dct', 'sampled_dct_seeded') else cabi_x.sampled_dft_workspace_bytes
        need = query(length, FEATURES, P, dtype)
        assert need > 0
        out_dtype = torch.float32 if seed_kind == 'int' else None                      # ('dft' only)
        odt = dtype if kind == 'dct' or out_dtype is None else out_dtype
        shape = (P, FEATURES) if kind == 'dct' else (2, P, FEATURES)
        if seeded:
            rows_arg = (P, -3 - (1 << 64)) if seed_kind == 'int' else (P, word)
            middle = ((-3) & MASK, 0, P, 1.5) if seed_kind == 'int' else (0, word.data_ptr(), P, 1.5)
        else:
            rows_arg, middle = idx, (idx.data_ptr(), P, 1.5)
        kw = {'scale': 1.5}
        if kind == 'dft':
            kw['out_dtype'] = out_dtype
        if seed_kind == 'int':
            out = torch.empty(shape, dtype=odt, device=DEV)
            workspace = torch.empty(need + 64, dtype=torch.uint8, device=DEV)
            kw.update(out=out, workspace=workspace, stream=0x1234)
        calls = _record(monkeypatch, module.lib(), symbol)
        with torch.cuda.stream(side):
            got = _call(name, m, rows_arg, **kw)
        assert len(calls) == 1
        head = (CODE[dtype], m.data_ptr(), *lead, FEATURES, LD, *middle, *((CODE[odt], ) if kind == 'dft' else ()))
        if seed_kind == 'int':
            assert got is out
            assert calls[0] == (*head, out.data_ptr(), workspace.data_ptr(), need + 64, 0x1234)
        else:
            assert got.shape == shape and got.dtype == odt and got.device == m.device and got.is_contiguous()
            assert calls[0][:len(head)] == head
            op, wp, wb, stream = calls[0][len(head):]
            assert op == got.data_ptr() and wp != 0 and wp % 16 == 0 and wb == need and stream == side.cuda_stream


@pytest.mark.parametrize('seed_kind', ('int', 'word'))
@pytest.mark.parametrize('dtype', (torch.float32, torch.bfloat16), ids=('fp32', 'bf16'))
def test_the_arguments_of_the_column_sampling_calls(dtype, seed_kind, monkeypatch):
    """crs_gather: (dtype, x, rows, in_features, ld, seed, seed_device, nopairs, cap, out, workspace, workspace_bytes, stream); crs_scatter:
    (dtype, t, out_features, cap, seed, seed_device, in_features, nopairs, gw, workspace, workspace_bytes, stream); nopairs = 9"""
    side = torch.cuda.Stream(DEV)
    word = torch.tensor([77], dtype=torch.int64, device=DEV)
    seed = -3 - (1 << 64) if seed_kind == 'int' else word
    value, pointer = ((-3) & MASK, 0) if seed_kind == 'int' else (0, word.data_ptr())
    cap = cabi_x.crs_count(-3, FEATURES, 9) if seed_kind == 'int' else 9
    assert 1 <= cap <= 9
    x = _matrix(256, dtype)
    t = torch.zeros(24, cap, dtype=dtype, device=DEV)
    need_x, need_t = cabi_x.crs_workspace_bytes(256, FEATURES, 9, dtype), cabi_x.crs_workspace_bytes(24, FEATURES, 9, dtype)
    assert need_x > 0 and need_t > 0
    out_x, ws_x = torch.empty(256, cap, dtype=dtype, device=DEV), torch.empty(need_x + 64, dtype=torch.uint8, device=DEV)
    out_t, ws_t = torch.empty(24, FEATURES, dtype=dtype, device=DEV), torch.empty(need_t + 64, dtype=torch.uint8, device=DEV)
    gather = _record(monkeypatch, cabi_x.lib(), 'fewbit_hipx_crs_gather')
    scatter = _record(monkeypatch, cabi_x.lib(), 'fewbit_hipx_crs_scatter')
    with torch.cuda.stream(side):
        assert cabi_x.crs_gather(x, seed, 9, out=out_x, workspace=ws_x) is out_x
        assert cabi_x.crs_scatter(t, seed, FEATURES, 9, out=out_t, workspace=ws_t) is out_t
        fresh = cabi_x.crs_gather(x, seed, 9)
    assert gather[0] == (CODE[dtype], x.data_ptr(), 256, FEATURES, LD, value, pointer, 9, cap, out_x.data_ptr(), ws_x.data_ptr(), need_x + 64, side.cuda_stream)
    assert scatter == [(CODE[dtype], t.data_ptr(), 24, cap, value, pointer, FEATURES, 9, out_t.data_ptr(), ws_t.data_ptr(), need_t + 64, side.cuda_stream)]
    assert fresh.shape == (256, cap) and fresh.dtype == dtype and fresh.device == x.device
    assert gather[1][:9] == gather[0][:9] and gather[1][9] == fresh.data_ptr() and gather[1][11:] == (need_x, side.cuda_stream)


@pytest.mark.parametrize('name', IDX_WRAPPERS)
def test_idx_must_be_a_contiguous_int64_vector_on_the_device_of_the_matrix(name):
    text = 'idx must be a contiguous 1-D int64 tensor on the device of ' + ('x' if WRAPPERS[name][3] else 'm')
    m = _matrix(300 if WRAPPERS[name][3] else 256)
    for idx in (_idx().int(), torch.arange(2 * P, dtype=torch.int64, device=DEV)[::2], torch.arange(P, dtype=torch.int64), _idx().reshape(1, P)):
        assert _message(lambda: _call(name, m, idx)) == text


@pytest.mark.parametrize('name', DFT_WRAPPERS)
def test_out_dtype_is_fp32_or_the_dtype_of_the_matrix(name):
    zext = WRAPPERS[name][3]
    m = _matrix(300 if zext else 256, torch.bfloat16)
    text = f'out_dtype must be torch.float32 or the dtype of {"x" if zext else "m"} (got torch.float16)'
    assert _message(lambda: _call(name, m, _rows_arg(name), out_dtype=torch.float16)) == text


@pytest.mark.parametrize('name', PLAIN_WRAPPERS)
def test_a_plain_wrapper_refuses_300_rows_but_not_an_empty_call(name):
    kind = WRAPPERS[name][2]
    m = _matrix(300)
    assert _message(lambda: _call(name, m, _rows_arg(name))) == f'sampled_{kind}: no kernel for 300 rows ({ROWS} is needed)'
    # the rows are asked about before out
    assert _message(lambda: _call(name, m, _rows_arg(name), out=torch.empty(1, device=DEV))) == f'sampled_{kind}: no kernel for 300 rows ({ROWS} is needed)'
    # the matrix before the rows
    assert _message(lambda: _call(name, m.double(), _rows_arg(name))) == 'unsupported dtype torch.float64'
    assert _message(lambda: _call(name, m.cpu(), _rows_arg(name, seed=7) if WRAPPERS[name][4] else torch.arange(P))) == 'm must live on the GPU (got cpu)'
    assert _message(lambda: _call(name, m[None], _rows_arg(name))) == 'm must be 2-D with unit stride along its last dimension'
    # C answers an empty call before it looks at the rows
    empty = _call(name, m, _rows_arg(name, p=0))
    assert empty.shape == ((0, FEATURES) if kind == 'dct' else (2, 0, FEATURES)) and empty.dtype == m.dtype and empty.device == m.device
    torch.cuda.synchronize()


@pytest.mark.parametrize('name', ZEXT_WRAPPERS)
def test_a_zero_extended_wrapper_refuses_a_length_without_a_kernel_and_rows_outside_it(name):
    kind = WRAPPERS[name][2]
    no_kernel = f'sampled_{kind}_zext: no kernel for 300 rows ({ROWS} is needed; sampled_rows_ceil gives the next one)'
    assert _message(lambda: _call(name, _matrix(300), _rows_arg(name), length=300)) == no_kernel
    assert _message(lambda: _call(name, _matrix(300), _rows_arg(name, p=0), length=300)) == no_kernel                  # even when empty
    assert _message(lambda: _call(name, _matrix(600), _rows_arg(name))) == f'sampled_{kind}_zext: x has 600 rows, 1 .. rows = 512 are needed'
    assert _message(lambda: _call(name, _matrix(600), _rows_arg(name, p=0))) == f'sampled_{kind}_zext: x has 600 rows, 1 .. rows = 512 are needed'
    assert _message(lambda: _call(name, _matrix(0), _rows_arg(name))) == f'sampled_{kind}_zext: x has 0 rows, 1 .. rows = 512 are needed'
    # the length before the rows of x, both before out; the matrix before either
    assert _message(lambda: _call(name, _matrix(600), _rows_arg(name), length=300, out=torch.empty(1, device=DEV))) == no_kernel
    assert _message(lambda: _call(name, _matrix(600).double(), _rows_arg(name), length=300)) == 'unsupported dtype torch.float64'


@pytest.mark.parametrize('name', tuple(WRAPPERS))
def test_out_must_have_the_shape_and_dtype_of_the_result(name):
    _, _, kind, zext, _ = WRAPPERS[name]
    m = _matrix(300 if zext else 256, torch.bfloat16)
    shape = (P, FEATURES) if kind == 'dct' else (2, P, FEATURES)
    text = 'out must be a contiguous ' + (f'proj x features tensor of the dtype of {"x" if zext else "m"}' if kind == 'dct' else '2 x proj x features tensor of out_dtype')
    wrong_shape = torch.empty((P + 1, FEATURES) if kind == 'dct' else (P, FEATURES), dtype=torch.bfloat16, device=DEV)
    wrong_dtype = torch.empty(shape, dtype=torch.float32, device=DEV)
    strided = torch.empty((*shape[:-1], LD), dtype=torch.bfloat16, device=DEV)[..., :FEATURES]
    for out in (wrong_shape, wrong_dtype, strided):
        assert _message(lambda: _call(name, m, _rows_arg(name), out=out)) == text


def _seeded_calls():
    """every entry point that takes a seed, as (id, call of a seed)"""
    calls = [(name, lambda seed, name=name: _call(name, _matrix(300 if WRAPPERS[name][3] else 256), (P, seed))) for name in SEEDED_WRAPPERS]
    calls.append(('crs_gather', lambda seed: cabi_x.crs_gather(_matrix(256), seed, 9)))
    calls.append(('crs_scatter', lambda seed: cabi_x.crs_scatter(torch.zeros(24, 9, device=DEV), seed, FEATURES, 9)))
    calls.append(('sketch', lambda seed: cabi.sketch('rademacher', _matrix(256), P, seed)))
    return calls


@pytest.mark.parametrize('call', [c for _, c in _seeded_calls()], ids=[n for n, _ in _seeded_calls()])
def test_a_seed_tensor_is_one_int64_word_on_the_device_of_the_matrix(call):
    text = 'seed must be a one-element int64 tensor on the GPU'
    assert _message(lambda: call(torch.tensor([7], dtype=torch.int32, device=DEV))) == text
    assert _message(lambda: call(torch.tensor([7, 8], dtype=torch.int64, device=DEV))) == text
    assert _message(lambda: call(torch.tensor([7], dtype=torch.int64))) == text


@pytest.mark.parametrize('call', [c for _, c in _seeded_calls()], ids=[n for n, _ in _seeded_calls()])
def test_a_seed_word_on_another_device_is_refused(call):
    if torch.cuda.device_count() < 2:
        pytest.skip('a seed word on another device needs a second device')
    assert _message(lambda: call(torch.tensor([7], dtype=torch.int64, device='cuda:1'))) == 'tensors live on different devices (cuda:0 and cuda:1)'
