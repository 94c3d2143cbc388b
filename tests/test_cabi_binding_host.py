"""The ctypes binding is derived from include/tdr.h (textualdegremoval_amd/_lib.py): the parser on every construct the header uses,
its strictness, and the derived struct layouts against a C compiler on the header itself.  No GPU, the library is not loaded."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from textualdegremoval_amd import _lib
from textualdegremoval_amd._lib import c_fp, f32, i32, i64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DESC = 'typedef struct TdrXDesc { int N; const float* x; } TdrXDesc;\n'


def sig(text, name='f'):
    return _lib.parse(text)[1][name]


def fields(text, name='TdrS'):
    return _lib.parse(text)[0][name]._fields_


def test_comments_and_preprocessor_lines_are_stripped():
    structs, sigs = _lib.parse('/* int gone(void); */\n#ifndef X_H\n#define X_H\n#include <stdint.h>\n#ifdef __cplusplus\nextern "C" {\n#endif\n'
                               'int f(int a /* [N] or NULL; int b */);   // int gone2(void);\n#ifdef __cplusplus\n}\n#endif\n#endif\n')
    assert structs == {} and sigs == {'f': (i32, [i32])}


def test_prototype_over_several_lines():
    assert sig('int64_t f(const float* x, int64_t x_ns,\n          float eps, int N,\n          void* stream);') == (i64, [c_fp, i64, f32, i32, c_fp])


def test_void_parameter_list():
    assert sig('int f(void);') == (i32, []) and sig('int f( void );') == (i32, [])


def test_several_declarators_in_one_declaration():
    assert fields('typedef struct TdrS {\n    int N, Cin, H, W;\n    float scale, inv_scale, max_scale;\n    const void *w3, *w4;\n} TdrS;') == [
        ('N', i32), ('Cin', i32), ('H', i32), ('W', i32), ('scale', f32), ('inv_scale', f32), ('max_scale', f32), ('w3', c_fp), ('w4', c_fp)]


def test_several_declarations_on_one_line():
    assert fields('typedef struct TdrS { float* out; int64_t out_ns;  int Mpad; float *mu, *rs; int64_t* nbt; } TdrS;') == [
        ('out', c_fp), ('out_ns', i64), ('Mpad', i32), ('mu', c_fp), ('rs', c_fp), ('nbt', c_fp)]


def test_star_on_either_side():
    assert sig('int f(float* a, float *b, float * c, const void *d, float*e);') == (i32, [c_fp] * 5)


def test_pointer_to_const_pointer():
    assert sig('int f(const float* const* src, float* const* dst, int n);') == (i32, [c_fp, c_fp, i32])


def test_unsigned_uint8_double_pointers():
    assert sig('int f(unsigned* slot, const uint8_t* img, uint8_t* out, const double* window, double* ws, const int* idx, const int64_t* sizes);') \
        == (i32, [c_fp] * 7)


def test_const_char_pointer_return():
    assert sig('const char* f(void);') == (C.c_char_p, []) and sig('const char *f(void);') == (C.c_char_p, [])


def test_in_field_is_spelled_inp():
    assert fields('typedef struct TdrS { const float* in; int64_t in_ns; } TdrS;') == [('inp', c_fp), ('in_ns', i64)]
    for name in ('TdrConvDesc', 'TdrConvP16Desc', 'TdrWgradDesc'):
        names = [n for n, _ in getattr(_lib, name)._fields_]
        assert 'inp' in names and 'in' not in names


def test_struct_pointers_host_descriptors_device_addresses_and_opaque_handles():
    structs, sigs = _lib.parse(DESC + 'typedef struct TdrPackJob { int M; } TdrPackJob;\ntypedef struct TdrStepGuard { float scale; } TdrStepGuard;\n'
                               'typedef struct TdrComm TdrComm;\n'
                               'int a(const TdrXDesc* d, void* stream);\nint b(TdrXDesc* d);\nint c(TdrPackJob* job, const TdrPackJob* jobs_dev);\n'
                               'int d(const TdrStepGuard* guard, float* loss);\nint d2(double* sumsq, TdrStepGuard* guard);\n'
                               'int e(TdrComm** comm, int rank);\nint e2(const TdrComm* comm);\n')
    assert sigs['a'] == (i32, [C.POINTER(structs['TdrXDesc']), c_fp])
    assert sigs['a'][1][0] is sigs['b'][1][0] and sigs['a'][1][0]._type_ is structs['TdrXDesc']          # one class object each time
    assert sigs['c'] == (i32, [C.POINTER(structs['TdrPackJob']), c_fp])
    assert sigs['d'] == sigs['d2'] == (i32, [c_fp, c_fp]) and sigs['e'] == (i32, [c_fp, i32]) and sigs['e2'] == (i32, [c_fp])
    assert fields(DESC + 'typedef struct TdrS { const TdrXDesc* d; } TdrS;') == [('d', c_fp)]             # a field is an address, whatever it points to
    # the header itself: every descriptor by POINTER(its class), the six device-resident struct pointers as integers
    S = _lib.SIGNATURES
    assert S['tdr_pack_job_init'][1][0]._type_ is _lib.TdrPackJob and S['tdr_pack_weights_multi'][1][0] is c_fp
    for name, arg in (('tdr_l1_loss_guarded', 4), ('tdr_pixel_loss', 9), ('tdr_multi_copy_guarded', 6), ('tdr_grad_sumsq_guarded', 8),
                      ('tdr_adamw_step_guarded', 11)):
        assert S[name][1][arg] is c_fp, name
    descs = [v for k, v in vars(_lib).items() if k.startswith('Tdr') and k.endswith('Desc')]
    assert len(descs) == 14
    for d in descs:
        users = [n for n, (_, args) in S.items() if args and args[0] is C.POINTER(d)]
        assert users, d.__name__
    assert _lib.TdrWg1GroupEntry._fields_ == [(n, c_fp) for n in ('inp', 'dout', 'part', 'dbpart', 'g', 'db')]


@pytest.mark.parametrize('text, names', [
    ('int f(size_t n);', 'size_t n'),                                              # unknown scalar type
    ('typedef struct TdrS { int N; long stride; } TdrS;', 'long stride'),
    ('int f(TdrNoSuch* d);', 'TdrNoSuch* d'),                                      # pointer to an undeclared struct
    (DESC + 'int f(TdrXDesc d);', 'TdrXDesc d'),                                   # struct by value
    ('double f(void);', 'double'),                                                 # unknown return type
    ('int f(void* p, ...);', '...'),
    ('typedef int (*tdr_callback)(int code);', 'typedef int (*tdr_callback)(int code)'),       # statements of an unknown shape
    ('int f(int (*cb)(int));', 'int f(int (*cb)(int))'),
    ('typedef struct TdrS { int a[4]; } TdrS;', 'int a[4]'),
    ('typedef struct TdrA { int N; } TdrB;', 'TdrB'),
    ('int f(void)', 'int f(void)'),                                                # no terminating semicolon
    ('enum { A, B };', 'enum { A, B }'),
    ('static const int k = 3;', 'static const int k = 3'),
])
def test_unknown_types_and_statements_raise_and_name_the_text(text, names):
    with pytest.raises(_lib.TdrError) as e:
        _lib.parse('int ok(void);\n' + text)
    assert names in str(e.value), str(e.value)


def test_missing_header_raises_tdr_error_with_the_path(tmp_path):
    missing = str(tmp_path / 'include' / 'tdr.h')
    with pytest.raises(_lib.TdrError, match='tdr.h') as e:
        _lib.read_header(missing)
    assert missing in str(e.value)
    versionless = tmp_path / 'v.h'
    versionless.write_text('int tdr_version(void);\n')
    with pytest.raises(_lib.TdrError, match='TDR_ABI_VERSION'):
        _lib.read_header(str(versionless))
    assert os.path.samefile(_lib.HEADER_PATH, os.path.join(ROOT, 'include', 'tdr.h'))
    assert _lib.read_header(_lib.HEADER_PATH)[0] == _lib.ABI_VERSION


def test_struct_layouts_match_the_c_compiler(tmp_path):
    """sizeof and every offsetof of every struct the header defines, from the system C compiler on include/tdr.h itself (host only:
    nothing of the GPU toolchain, no process that opens the GPU), against the ctypes classes the binding derives."""
    cc = shutil.which('cc') or shutil.which('gcc') or shutil.which('clang')
    if cc is None:
        pytest.skip('no C compiler on PATH')
    structs = _lib.parse(open(_lib.HEADER_PATH).read())[0]
    assert len(structs) == 17 and all(getattr(_lib, k)._fields_ == v._fields_ for k, v in structs.items())
    c_name = {v: k for k, v in _lib._PY_FIELD.items()}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "tdr.h"', 'int main(void) {']
    for name, s in structs.items():
        lines.append(f'    printf("{name} sizeof %zu\\n", sizeof({name}));')
        lines += [f'    printf("{name} {n} %zu\\n", offsetof({name}, {c_name.get(n, n)}));' for n, _ in s._fields_]
    lines += ['    return 0;', '}']
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines) + '\n')
    exe = str(tmp_path / 'layout')
    subprocess.run([cc, '-std=c99', '-Wall', '-Werror', '-I', os.path.dirname(_lib.HEADER_PATH), str(src), '-o', exe], check=True)
    got = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    want = []
    for name, s in structs.items():
        cls = getattr(_lib, name)
        want.append(f'{name} sizeof {C.sizeof(cls)}')
        want += [f'{name} {n} {getattr(cls, n).offset}' for n, _ in s._fields_]
    assert got == want
    assert C.sizeof(_lib.TdrConvDesc) == 248 and C.sizeof(_lib.TdrPackJob) == 72 and C.sizeof(_lib.TdrStepGuard) == 40
