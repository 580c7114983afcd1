"""CPU: libiamx.so loads and exports exactly the C ABI include/iamx.h declares."""
import ctypes
import os
import re

import pytest

from conftest import REPO


def _declared():
    text = open(os.path.join(REPO, 'include', 'iamx.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(iamx_[a-z0-9_]+)\s*\(', text)))


def test_header_and_binding_table_agree():
    from imageanalysis_amd import _lib
    assert sorted(_lib.SIGNATURES) == _declared()


def test_binding_table_pins():
    """entries typed out by hand (from the table _lib.py carried before it parsed the header) that
    together use every type rule of the parser"""
    from ctypes import c_char_p, c_double, c_float, c_int, c_int64, c_uint64, c_void_p
    from imageanalysis_amd._lib import SIGNATURES
    assert SIGNATURES['iamx_last_error'] == (c_char_p, [])
    assert SIGNATURES['iamx_yaw_feedback_new'] == (c_void_p, [c_int, c_void_p])
    assert SIGNATURES['iamx_yaw_feedback_free'] == (None, [c_void_p])
    assert SIGNATURES['iamx_desc_padded_rows'] == (c_int64, [c_int64])
    assert SIGNATURES['iamx_comm_init'] == (c_int, [c_int, c_int, c_void_p, c_void_p])
    assert SIGNATURES['iamx_image_equalize_resize'] == (
        c_int, [c_void_p, c_int, c_int, c_int, c_float, c_double, c_void_p, c_int64, c_void_p, c_void_p])
    assert SIGNATURES['iamx_verify_pairs'] == (
        c_int, [c_void_p, c_void_p, c_int, c_int64, c_int, c_void_p, c_int, c_uint64] + [c_void_p] * 5)
    assert SIGNATURES['iamx_knn2sym_exact'] == (
        c_int, [c_void_p] * 4 + [c_int64] + [c_void_p] * 8 + [c_int, c_double] + [c_void_p] * 13
        + [c_int64, c_int, c_void_p])
    assert len(SIGNATURES) == len(_declared())


def test_parser_reads_the_spellings_a_header_may_use():
    from ctypes import c_char_p, c_double, c_float, c_int, c_int64, c_uint64, c_void_p
    from imageanalysis_amd._lib import parse_header
    table = parse_header('''
        #include <stdint.h>
        #ifdef __cplusplus
        extern "C" {
        #endif
        #define IAMX_N (1 << 4)   /* iamx_in_a_comment(int) */
        // int iamx_in_a_line_comment(unsigned n);
        int iamx_three_lines(const uint8_t *src, int64_t n,   /* rows */
                             double scale,
                             void *stream);
        int64_t iamx_unnamed(int, int64_t, const float *, uint64_t);
        int iamx_consts(const int n, int32_t const m, float const *p, const double x, float f);
        int iamx_arrays(double K[9], const float xy[][2], int n);
        void *iamx_handle(void **out, const int32_t *const *rows);
        const char *iamx_text(void);
        void iamx_nothing ( void ) ;
        #ifdef __cplusplus
        }
        #endif
    ''')
    assert table == {
        'iamx_three_lines': (c_int, [c_void_p, c_int64, c_double, c_void_p]),
        'iamx_unnamed': (c_int64, [c_int, c_int64, c_void_p, c_uint64]),
        'iamx_consts': (c_int, [c_int, c_int, c_void_p, c_double, c_float]),
        'iamx_arrays': (c_int, [c_void_p, c_void_p, c_int]),
        'iamx_handle': (c_void_p, [c_void_p, c_void_p]),
        'iamx_text': (c_char_p, []),
        'iamx_nothing': (None, []),
    }


@pytest.mark.parametrize('header, culprit', [
    ('int iamx_f(const float *p, unsigned n);', 'unsigned n'),
    ('int iamx_f(size_t n, void *stream);', 'size_t n'),
    ('int iamx_f(struct iamx_box b);', 'struct iamx_box b'),
    ('int iamx_f(iamx_box_t b);', 'iamx_box_t b'),
    ('int iamx_f(void (*done)(int), int n);', '(*done)'),
    ('int iamx_f(int (*cmp)(const void *, const void *));', '(*cmp)'),
    ('int iamx_f();', "''"),              # C: unspecified parameters, not none
    ('int iamx_f(int n, ...);', '...'),
    ('unsigned iamx_f(int n);', 'unsigned'),
    ('struct iamx_box iamx_f(int n);', 'struct iamx_box'),
    ('int iamx_f(int n);\nint iamx_g(void);\nint iamx_f(int n);', 'twice'),
    ('int iamx_f(int n)\nint iamx_g(void);', 'iamx_g'),
    ('static inline int iamx_f(int n) { return n; }', 'return n'),
    ('typedef int (*iamx_cb)(int);\nint x = iamx_f(3);', 'iamx_f(3)'),
])
def test_parser_rejects_what_it_has_no_rule_for(header, culprit):
    from imageanalysis_amd._lib import IamxError, parse_header
    with pytest.raises(IamxError) as e:
        parse_header(header)
    assert 'iamx_f' in str(e.value) and culprit in str(e.value)


def test_missing_header_is_named(monkeypatch, tmp_path):
    from imageanalysis_amd import _lib
    monkeypatch.setattr(_lib, 'HEADER_PATH', str(tmp_path / 'include' / 'iamx.h'))
    with pytest.raises(_lib.IamxError, match=re.escape(str(tmp_path / 'include' / 'iamx.h'))):
        _lib._signatures()


def test_import_needs_neither_torch_nor_the_library():
    import subprocess
    import sys
    code = ("import sys; sys.modules['torch'] = None; import os; os.environ['IAMX_LIB'] = '/nonexistent/libiamx.so'\n"
            "from imageanalysis_amd import _lib; assert len(_lib.SIGNATURES) > 100")
    subprocess.check_call([sys.executable, '-c', code], cwd=REPO)


def test_library_exports_every_symbol():
    from imageanalysis_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    h = ctypes.CDLL(_lib.LIB_PATH)
    for name in _declared():
        assert hasattr(h, name), name
    L = _lib.lib()
    assert L.iamx_version() >= 100
    assert L.iamx_arch() == b'gfx950'
    assert L.iamx_desc_padded_rows(1) == 128 and L.iamx_desc_padded_rows(128) == 128
    assert L.iamx_desc_padded_rows(129) == 256 and L.iamx_desc_padded_rows(0) == 0
    assert L.iamx_knn2_wg_per_pair(4096) == 16 and L.iamx_knn2_wg_per_pair(1) == 1


def test_argument_checks_do_not_need_a_gpu():
    from imageanalysis_amd import _lib
    L = _lib.lib()
    rc = L.iamx_knn2_l2_u8(None, None, 4, None, None, 4, None, None, None)
    assert rc == -1 and b'null pointer' in L.iamx_last_error()
    rc = L.iamx_ba_residual(None, 1, None, 1, None, None, None, 0, None, None, None)
    assert rc == -1
    assert L.iamx_comm_allgather(None, None, None, 16, None) == -1
    assert L.iamx_knn2sym_sweep(*([None] * 9), 1, 1, 2, None, None, None, None) == -1


def test_product_has_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from imageanalysis_amd import _lib
    with pytest.raises(_lib.IamxError):
        _lib.require_gpu()


def test_product_never_imports_the_oracle():
    """oracle/ is test infrastructure: nothing under imageanalysis_amd/ may import or load it."""
    import re
    pkg = os.path.join(REPO, 'imageanalysis_amd')
    pat = re.compile(r'^\s*(from|import)\s+oracle\b|oracle[/.]cpu_ref|liboracle|oracle/_ref', re.M)
    for root, _dirs, files in os.walk(pkg):
        for f in files:
            if f.endswith(('.py', '.hip', '.h', '.sh')):
                text = open(os.path.join(root, f)).read()
                assert not pat.search(text), os.path.join(root, f)
