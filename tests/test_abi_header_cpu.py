"""CPU: stereo_rcnn_amd/_lib.py derives its ctypes table (constants, structures, signatures) from include/srcnn_hip.h.  Checked here:
the structures' layout against what the host C compiler makes of the same header, the parser on a pinned snippet with one of each
construct the header uses (expected ctypes objects written out by hand) and on text it must refuse, and the typing convention
(struct pointers, *_host arrays, the explicit table, c_void_p for the rest) over every argument of the real header."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from stereo_rcnn_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'srcnn_hip.h')
P = ctypes.POINTER


# ---------------------------------------------------------------------------------------------- layout against a compiler
def test_structure_layout_is_the_c_compilers(tmp_path):
    cc = shutil.which('cc')
    assert cc, 'no host C compiler (cc) on PATH: the layout cannot be checked'
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "srcnn_hip.h"', 'int main(void) {']
    for cname, cls in _lib.HEADER.structs.items():
        lines.append('    printf("%s - %%zu 0\\n", sizeof(%s));' % (cname, cname))
        for field, _ in cls._fields_:
            lines.append('    printf("%s %s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s *)0)->%s));'
                         % (cname, field, cname, field, cname, field))
    lines += ['    return 0;', '}', '']
    src, exe = tmp_path / 'layout.c', tmp_path / 'layout'
    src.write_text('\n'.join(lines))
    subprocess.check_call([cc, '-std=c99', '-Wall', '-Werror', '-I', os.path.dirname(HEADER), str(src), '-o', str(exe)])
    out = subprocess.check_output([str(exe)]).decode().split('\n')
    got = {tuple(ln.split()[:2]): tuple(int(v) for v in ln.split()[2:]) for ln in out if ln}
    want = {}
    for cname, cls in _lib.HEADER.structs.items():
        want[(cname, '-')] = (ctypes.sizeof(cls), 0)
        for field, _ in cls._fields_:
            want[(cname, field)] = (getattr(cls, field).offset, getattr(cls, field).size)
    assert len(_lib.HEADER.structs) == 12 and len(want) == 12 + 219
    assert got == want, sorted(set(got.items()) ^ set(want.items()))
    assert want[('srcnn_conv_desc', '-')] == (288, 0) and want[('srcnn_conv_desc', 'up_W')] == (280, 4)
    assert want[('srcnn_prep_layer', '-')] == (200, 0)
    assert want[('srcnn_train_weight_desc', '-')] == (6 * 8 + 4 * 4, 0)             # six pointers, four ints
    assert want[('srcnn_train_fold_desc', '-')] == ((4 * 3 + 6) * 8 + (3 + 6) * 4 + 4, 0) == (184, 0)   # 18 pointers, 9 ints, tail padding


# ---------------------------------------------------------------------------------------------- the parser on pinned text
SNIPPET = '''
/* a pinned header: one of each construct include/srcnn_hip.h uses; this comment holds a ; and SRCNN_API int not_this(void); */
#ifndef SRCNN_SNIPPET_H
#define SRCNN_SNIPPET_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif
#define SRCNN_X (-3)
#define SRCNN_COLS 32
typedef void *srcnn_stream_t; /* hipStream_t */
#define SRCNN_API __attribute__((visibility("default")))
SRCNN_API int srcnn_version(void);   /* 310 = a, b; 300 = c */
SRCNN_API const char *srcnn_last_error(void);
typedef struct srcnn_conv_desc {
    const float *w;        /* (Cout) or NULL */
    float a[4], b[4];
    int x, y;
    void *p[3];
    float *dx, *dw;
    long long plane;
    double s;
    const signed char *flags;
} srcnn_conv_desc;
SRCNN_API size_t srcnn_conv2d_workspace_bytes(const srcnn_conv_desc *d);
SRCNN_API void srcnn_program_destroy(void *program);
SRCNN_API const void *srcnn_device_word(void);
SRCNN_API int srcnn_run(const float *const *x_host, const int *n_host,
                        long long rows, unsigned flags /* bits, see above; a comment with a , and a ) inside the list */,
                        const unsigned char *img, const unsigned *mask, const srcnn_conv_desc *d, double s, float t,
                        void *workspace, size_t workspace_bytes, srcnn_stream_t stream);
SRCNN_API int srcnn_stream_create(int dedicated_queue, srcnn_stream_t *stream);
#ifdef __cplusplus
}
#endif
#endif /* SRCNN_SNIPPET_H */
'''
SNIPPET_HOST_ARRAYS = {'srcnn_stream_create': ('stream',), 'srcnn_run': ('mask',)}


def test_parser_on_pinned_text():
    h = _lib.parse_header(SNIPPET, SNIPPET_HOST_ARRAYS)
    assert h.constants == {'X': -3, 'COLS': 32}
    assert list(h.structs) == ['srcnn_conv_desc']
    S = h.structs['srcnn_conv_desc']
    assert S.__name__ == 'ConvDesc' and issubclass(S, ctypes.Structure)
    v, f, i = ctypes.c_void_p, ctypes.c_float, ctypes.c_int
    want = [('w', v), ('a', f * 4), ('b', f * 4), ('x', i), ('y', i), ('p', v * 3), ('dx', v), ('dw', v),
            ('plane', ctypes.c_longlong), ('s', ctypes.c_double), ('flags', v)]
    assert [n for n, _ in S._fields_] == [n for n, _ in want]
    assert all(t is w for (_, t), (_, w) in zip(S._fields_, want)), S._fields_
    want = {
        'srcnn_version': (i, []),
        'srcnn_last_error': (ctypes.c_char_p, []),
        'srcnn_conv2d_workspace_bytes': (ctypes.c_size_t, [P(S)]),
        'srcnn_program_destroy': (None, [v]),
        'srcnn_device_word': (v, []),
        'srcnn_run': (i, [P(v), P(i), ctypes.c_longlong, ctypes.c_uint, v, P(ctypes.c_uint), P(S), ctypes.c_double, f,
                          v, ctypes.c_size_t, v]),
        'srcnn_stream_create': (i, [i, P(v)]),
    }
    assert list(h.signatures) == list(want)
    for name, (res, args) in want.items():
        assert h.signatures[name][0] is res, name
        assert len(h.signatures[name][1]) == len(args) and all(a is b for a, b in zip(h.signatures[name][1], args)), name
    # without the table the two listed arguments are device pointers like any other
    plain = _lib.parse_header(SNIPPET).signatures
    assert plain['srcnn_stream_create'][1][1] is v and plain['srcnn_run'][1][5] is v


def _with(decl):
    return SNIPPET.replace('SRCNN_API int srcnn_version(void);', decl)


REFUSALS = {   # what: (header text, host-array table, what the message must hold)
    # the three the binding must never let through
    'unknown base type': (_with('SRCNN_API int srcnn_f(int n, uint64_t bytes);'), {},
                          r"unknown base type 'uint64_t'.*srcnn_f\(int n, uint64_t bytes\)"),
    'table names a missing argument': (SNIPPET, {'srcnn_program_destroy': ('handle',)},
                                       r'names handle.*srcnn_program_destroy\(void \*program\)'),
    '_host on a value': (_with('SRCNN_API int srcnn_f(const float *x, int n_host);'), {},
                         r'pointer.*int n_host in .*srcnn_f\(const float \*x, int n_host\)'),
    # and the rest of what is refused, never skipped
    'table names a value': (SNIPPET, {'srcnn_run': ('rows',)}, r'pointer.*long long rows in .*srcnn_run'),
    'table names a missing function': (SNIPPET, {'srcnn_missing': ('a',)}, r'functions the header lacks: srcnn_missing'),
    '_host on void *': (_with('SRCNN_API int srcnn_f(void *x_host);'), {}, r'sized type.*void \*x_host'),
    'field twice': (SNIPPET.replace('int x, y;', 'int x, a;'), {}, r'does not split.*srcnn_conv_desc'),
    'function twice': (_with('SRCNN_API int srcnn_last_error(void);'), {}, r"duplicate name 'srcnn_last_error'"),
    'macro twice': (_with('#define SRCNN_X 4'), {}, r"duplicate name 'X'.*#define SRCNN_X 4"),
    'macro 4u': (_with('#define SRCNN_Y 4u'), {}, r'not an integer.*#define SRCNN_Y 4u'),
    'no SRCNN_API': (_with('int srcnn_f(int n);'), {}, r'does not split.*int srcnn_f\(int n\)'),
    'unnamed argument': (_with('SRCNN_API int srcnn_f(int);'), {}, r'does not split.*srcnn_f\(int\)'),
    'function pointer': (_with('SRCNN_API int srcnn_f(int (*cb)(int));'), {}, r'does not split.*srcnn_f'),
    'array argument': (_with('SRCNN_API int srcnn_f(const float x[4]);'), {}, r'does not split.*srcnn_f'),
    'void value': (_with('SRCNN_API int srcnn_f(void v);'), {}, r'void.*srcnn_f\(void v\)'),
    'struct without typedef': (_with('struct srcnn_s { int a; };'), {}, r'does not split.*struct srcnn_s'),
}


@pytest.mark.parametrize('what', list(REFUSALS))
def test_parser_refuses_with_the_text(what):
    text, table, message = REFUSALS[what]
    with pytest.raises(ValueError, match=re.compile(message, re.S)):
        _lib.parse_header(text, table)


def test_a_missing_header_is_an_error_that_names_the_path(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, 'HEADER_PATH', str(tmp_path / 'include' / 'srcnn_hip.h'))
    with pytest.raises(RuntimeError, match=re.escape(str(tmp_path / 'include' / 'srcnn_hip.h'))):
        _lib._read_header()


# ---------------------------------------------------------------------------------------------- the convention on the real header
def _declarations():
    """The header's declarations by a reading of its own: {function: [(argument text, argument name)]}."""
    text = re.sub(r'/\*.*?\*/', ' ', open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r'SRCNN_API\s+[^;()]*?(\w+)\s*\(([^()]*)\)\s*;', text):
        args = [] if m.group(2).strip() == 'void' else [' '.join(a.split()) for a in m.group(2).split(',')]
        out[m.group(1)] = [(a, re.findall(r'\w+', a)[-1]) for a in args]
    return out


def test_the_real_header_follows_the_convention():
    decls = _declarations()
    assert sorted(decls) == _lib.declared_symbols() and len(decls) == 120
    structs = _lib.HEADER.structs
    assert [s.__name__ for s in structs.values()] == [
        'ConvDesc', 'ConvBwdDesc', 'ConvFwdF16x3Desc', 'TrainWeightDesc', 'TrainFoldDesc', 'AnchorTargetParams',
        'ProposalTargetParams', 'PrepLayer', 'GtSlot', 'TrainImage', 'KittiSplit', 'KittiMatchDesc']
    assert all(getattr(_lib, s.__name__) is s for s in structs.values())
    scalars = {'int': ctypes.c_int, 'unsigned': ctypes.c_uint, 'long long': ctypes.c_longlong, 'float': ctypes.c_float,
               'double': ctypes.c_double, 'size_t': ctypes.c_size_t}
    table = {(fn, a) for fn, names in _lib._HOST_ARRAYS.items() for a in names}
    assert len(table) == 15
    host, listed = 0, set()
    for fn, args in decls.items():
        argtypes = _lib._SIGNATURES[fn][1]
        assert len(argtypes) == len(args), fn
        for (text, name), t in zip(args, argtypes):
            struct = [s for c, s in structs.items() if re.search(r'\b%s\b' % c, text)]
            if '*' not in text and 'srcnn_stream_t' not in text:
                assert t is scalars[text[:-len(name)].strip()], (fn, text)
            elif struct:
                assert text.count('*') == 1 and t is P(struct[0]), (fn, text)
            elif name.endswith('_host') or (fn, name) in table:
                assert issubclass(t, ctypes._Pointer) and t._type_ in set(scalars.values()) | {ctypes.c_void_p}, (fn, text)
                assert (t._type_ is ctypes.c_void_p) == (text.count('*') == 2 or 'srcnn_stream_t *' in text), (fn, text)
                if name.endswith('_host'):
                    host += 1
                else:
                    listed.add((fn, name))
            else:
                assert t is ctypes.c_void_p, (fn, text)
    assert listed == table and host == 33      # exactly the table's entries are typed without the suffix


def test_every_integer_macro_is_an_attribute():
    text = open(HEADER).read()
    macros = re.findall(r'^#define[ \t]+(\w+)(?:[ \t]+(\S.*?))?[ \t]*$', text, re.M)
    ints = {n[len('SRCNN_'):]: int(v.strip('()')) for n, v in macros if re.fullmatch(r'\(-?\d+\)|-?\d+', v)}
    assert len(ints) == 38 and len(macros) == 40 and ints == _lib.HEADER.constants
    for name, v in ints.items():
        assert getattr(_lib, name) == v and type(getattr(_lib, name)) is int
    assert not hasattr(_lib, 'API') and not hasattr(_lib, 'HIP_H')
    # a few written out, the by-products among them
    assert (_lib.OK, _lib.ERR_ARG, _lib.ERR_HIP, _lib.ERR_WORKSPACE) == (0, -1, -2, -3)
    assert (_lib.FMT_F32, _lib.FMT_SPLIT16, _lib.REC_COLS, _lib.KITTI_MAX_DET, _lib.KITTI_COLS) == (0, 1, 32, 4096, 13)
    assert (_lib.SMOOTH_L1_MAX_D, _lib.SMOOTH_L1_MAX_SEL, _lib.OVERLAY_MAX_OFFSET) == (64, 1024, 1 << 20)
    from stereo_rcnn_amd import distributed, kitti_eval
    assert distributed.REC_COLS is _lib.REC_COLS and kitti_eval.MAX_DET_PER_FRAME is _lib.KITTI_MAX_DET
