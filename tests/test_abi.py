"""The C-ABI shared library: loads, exports every symbol include/lime_hip.h declares, rejects bad
arguments before touching the GPU.  No compute calls here (CPU only)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from lime_cikm25_amd import _lib
from lime_cikm25_amd._header import Header
from lime_cikm25_amd.build import build_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'lime_hip.h')


@pytest.fixture(scope='module')
def lib():
    build_library()
    return _lib.load()


def declared_symbols():
    text = open(HEADER).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(lime_[a-z0-9_]+)\s*\(', text)))


def test_header_and_binding_agree(lib):
    names = declared_symbols()
    assert len(names) >= 15
    assert sorted(_lib.SIGNATURES) == names
    for n in names:
        assert getattr(lib, n) is not None


def test_abi_version(lib):
    header = open(HEADER).read()
    declared = int(re.search(r'#define\s+LIME_ABI_VERSION\s+(\d+)', header).group(1))
    assert lib.lime_abi_version() == _lib.ABI_VERSION == declared


def _gcc(tmp_path, source, *flags):
    if shutil.which('gcc') is None:
        pytest.skip('no gcc')
    src = tmp_path / 'abi.c'
    src.write_text(source)
    return subprocess.run(['gcc', '-std=c11', '-Werror', *flags, str(src)], capture_output=True, text=True, cwd=tmp_path)


def test_every_struct_matches_the_header_field_by_field(tmp_path):
    """sizeof, and the offset and size of EVERY field, of every struct the reader found against what gcc gives it."""
    assert len(_lib.STRUCTS) >= 12
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % HEADER, 'int main(void) {']
    for cname, st in _lib.STRUCTS.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        lines += ['printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (cname, f, cname, f, cname, f) for f, _ in st._fields_]
    r = _gcc(tmp_path, '\n'.join(lines + ['return 0; }']), '-o', 'abi')
    assert r.returncode == 0, r.stderr[-3000:]
    got = subprocess.run([str(tmp_path / 'abi')], check=True, capture_output=True, text=True).stdout.splitlines()
    want = []
    for cname, st in _lib.STRUCTS.items():
        want.append('%s %d' % (cname, ctypes.sizeof(st)))
        want += ['%s.%s %d %d' % (cname, f, getattr(st, f).offset, getattr(st, f).size) for f, _ in st._fields_]
    assert got == want


C_SCALAR = {ctypes.c_int32: 'int32_t', ctypes.c_int64: 'int64_t', ctypes.c_uint32: 'uint32_t', ctypes.c_uint64: 'uint64_t',
            ctypes.c_float: 'float'}


def signature_unit(signatures):
    """A C unit that initialises one function pointer per entry with the header's own function.  The pointer's scalar parameter and
    return types are spelled from the DERIVED ctypes classes, its pointer types as the header's text: the unit compiles under -Werror
    only if every entry has the count, the order and every scalar class and width the C compiler sees in the header."""
    lines = ['#include "%s"' % HEADER]
    for name, (res, args) in sorted(signatures.items()):
        ret, params = _lib.C_TYPES[name]
        spelled = [C_SCALAR.get(cls, text) for cls, text in zip(args, params)]
        lines.append('%s (*const p_%s)(%s) = %s;' % (C_SCALAR.get(res, ret), name, ', '.join(spelled) or 'void', name))
    return '\n'.join(lines) + '\n'


def test_every_signature_is_what_the_c_compiler_sees(tmp_path):
    assert len(_lib.SIGNATURES) >= 121 and sorted(_lib.SIGNATURES) == sorted(_lib.C_TYPES)
    for name, (res, args) in _lib.SIGNATURES.items():
        assert len(args) == len(_lib.C_TYPES[name][1]), name
    r = _gcc(tmp_path, signature_unit(_lib.SIGNATURES), '-fsyntax-only')
    assert r.returncode == 0, r.stderr[-3000:]


def _narrowed(args):
    i = args.index(ctypes.c_int64)
    return args[:i] + [ctypes.c_int32] + args[i + 1:]


@pytest.mark.parametrize('name,wrong', [
    ('lime_negative_sample', _narrowed),                              # an int64_t taken for an int32_t
    ('lime_token_attention_bwd_f32', lambda args: args[:-1]),         # an argument dropped
    ('lime_adam_f32', lambda args: args[:5] + [ctypes.c_int32] + args[6:]),   # an int32_t where the header has a float
])
def test_a_wrong_signature_does_not_compile(tmp_path, name, wrong):
    """The control of the test above: its generator, fed ONE deliberately wrong entry, must be refused by the compiler."""
    res, args = _lib.SIGNATURES[name]
    assert wrong(list(args)) != args
    r = _gcc(tmp_path, signature_unit(dict(_lib.SIGNATURES, **{name: (res, wrong(list(args)))})), '-fsyntax-only')
    assert r.returncode != 0 and 'p_' + name in r.stderr, r.stderr[-3000:]


SMALL = '''/* a comment
   over two lines */
#ifndef SMALL_H
#define SMALL_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define SMALL_N 3   // a line comment
typedef enum { SMALL_OK = 0, SMALL_ERR = -1 } small_status;
enum { SMALL_A, SMALL_B, SMALL_C = 0x10, SMALL_D, SMALL_E = SMALL_N };
typedef struct small_tag {
    const float* a[SMALL_N];
    int32_t M, N, *p;
    char name[8];
    uint64_t const seed;
} small_args;
int small_version(void);
const char* small_name(void);
int64_t small_run(const small_args* args, small_args const* more, const uint8_t* mask,
                  int n, float scale,
                  uint32_t site, void* stream);
#ifdef __cplusplus
}
#endif
#endif
'''


def test_the_reader_on_every_form_the_header_uses():
    from ctypes import POINTER, c_char, c_char_p, c_float, c_int32, c_int64, c_uint32, c_uint64, c_void_p
    h = Header(SMALL)
    assert h.constants == dict(SMALL_N=3, SMALL_OK=0, SMALL_ERR=-1, SMALL_A=0, SMALL_B=1, SMALL_C=16, SMALL_D=17, SMALL_E=3)
    st = h.structs['small_args']
    assert list(h.structs) == ['small_args'] and st.__name__ == 'small_args'
    assert st._fields_ == [('a', c_void_p * 3), ('M', c_int32), ('N', c_int32), ('p', c_void_p), ('name', c_char * 8), ('seed', c_uint64)]
    assert h.signatures == {'small_version': (c_int32, []), 'small_name': (c_char_p, []),
                            'small_run': (c_int64, [POINTER(st), POINTER(st), c_void_p, c_int32, c_float, c_uint32, c_void_p])}
    assert h.c_types['small_run'] == ('int64_t', ['const small_args*', 'small_args const*', 'const uint8_t*', 'int', 'float', 'uint32_t', 'void*'])


@pytest.mark.parametrize('bad,line', [
    ('int f(int a);\n\nvoid g(int a);\n', 3),                      # a return type without a ctypes class
    ('int f(double x);\n', 1),                                     # a scalar outside the table
    ('/* c\n */\ntypedef struct { int a; double b; } s;\n', 3),
    ('typedef int (*callback)(int);\n', 1),
    ('int f(int a[3]);\n', 1),
    ('int f(int32_t);\n', 1),                                      # an unnamed parameter
    ('enum { A = 1 << 2 };\n', 1),
    ('\n#define N (1 + 2)\n', 2),
    ('#if FOO\nint f(void);\n#endif\n', 1),
    ('int f(void);\nint g(void)\n', 2),                            # no terminating semicolon
])
def test_the_reader_raises_on_what_it_cannot_read_and_names_the_line(bad, line):
    with pytest.raises(ValueError, match=r'^x\.h:%d: ' % line):
        Header(bad, 'x.h')


def test_missing_header_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, 'HEADER_PATH', str(tmp_path / 'nope.h'))
    with pytest.raises(_lib.LimeHipError, match='nope.h is missing'):
        _lib._read_header()


def test_bad_arguments_are_rejected_without_a_launch(lib):
    assert lib.lime_linear_f32(None, None) == -1
    assert b'NULL' in lib.lime_last_error_string()
    a = _lib.LinearArgs()
    assert lib.lime_linear_f32(ctypes.byref(a), None) == -1
    assert lib.lime_bucketize_f32(None, None, 4, None) == -1
    for entry, block, field in ((lib.lime_token_attention_f32, _lib.TokenAttentionArgs, 'form'),
                                (lib.lime_token_attention_bwd_f32, _lib.TokenAttentionBwdArgs, 'entry')):
        assert entry(None, None) == -1
        assert b'NULL' in lib.lime_last_error_string()
        a = block()
        assert entry(ctypes.byref(a), None) == -1
        for bad in (-1, max(_lib.ATTN_FORM.values()) + 1 if field == 'form' else max(_lib.BWD_ATTN_ENTRY.values()) + 1):
            setattr(a, field, bad)
            assert entry(ctypes.byref(a), None) == -1
            assert ('%s %d' % (field, bad)).encode() in lib.lime_last_error_string()
    assert lib.lime_pad_heads_f32(None, 1, None, 1, 1, 1, 1, 1, None) == -1
    assert lib.lime_multi_copy(None, 3, None) == -1
    assert lib.lime_multi_copy(None, 0, None) == 0
    assert lib.lime_multi_copy(None, 33, None) == -1
    assert lib.lime_gather_rows_multi(None, 4, None, 2, None) == -1
    assert lib.lime_gather_rows_multi(None, 0, None, 2, None) == 0
    # the bf16 encoder-block entry points: NULL / unsupported shapes are refused before any launch
    assert lib.lime_encoder_ffn_bf16(None, None) == -1 and lib.lime_encoder_block_bf16(None, None) == -1 and lib.lime_inproj_bf16(None, None) == -1
    assert lib.lime_encoder_ffn_bf16(ctypes.byref(_lib.FfnBf16Args()), None) == -1
    assert lib.lime_ffn_pack_bf16(None, 300, None, None, 512, 300, 512, None, None, None) == -1
    assert lib.lime_ffn_bf16_model_columns() == 304
    assert lib.lime_ffn_pack_bf16_size(512, 0) == 512 * 320 and lib.lime_ffn_pack_bf16_size(512, 1) == 512 * 304
    assert lib.lime_oproj_pack_bf16_size() == 10 * 304 * 32 and lib.lime_inproj_pack_bf16_size(960) == 960 * 320
    assert lib.lime_sage_mean_f32(None, None, None, 1, 1, 1, 1, 1, None) == -1
    with pytest.raises(_lib.LimeHipError):
        _lib.check(-1, 'x')


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setattr(_lib, 'LIB_PATH', str(tmp_path / 'nope.so'))
    with pytest.raises(_lib.LimeHipError):
        _lib.load()


def test_ops_refuse_cpu_tensors():
    import torch
    from lime_cikm25_amd import ops
    with pytest.raises(TypeError):
        ops.linear(torch.zeros(4, 8), torch.zeros(3, 8))
