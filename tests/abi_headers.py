"""The one reader of the C headers under include/ and the one check of a record of ``_lib.EXTENSIONS`` against its header
(tests/test_abi_headers.py runs it for every record; the per-extension CPU tests use the reader for what is specific to them)."""
import ctypes
import os
import re

from conftest import ROOT

SCALARS = {'void': None, 'int': ctypes.c_int32, 'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64, 'float': ctypes.c_float,
           'double': ctypes.c_double}


def source_of(header):
    """the text of include/<header> without its comments"""
    return re.sub(r'/\*.*?\*/|//[^\n]*', '', open(os.path.join(ROOT, 'include', header)).read(), flags=re.S)


def declared_symbols(header):
    return sorted(set(re.findall(r'\b(dcf_[a-z0-9_]+)\s*\(', source_of(header))))


def params_of(header, name):
    """-> (the parameter declarations of ``name`` with single blanks, e.g. 'const uint16_t* vid'; its return type)"""
    m = re.search(r'^[ \t]*([\w \t*]+?)[ \t]*\b' + name + r'\s*\((.*?)\)\s*;', source_of(header), flags=re.S | re.M)
    assert m, f'{name} is not declared in {header}'
    return [' '.join(p.split()) for p in m.group(2).split(',') if p.strip() and p.strip() != 'void'], ' '.join(m.group(1).split())


def param_names(header, name):
    return [p.split()[-1].lstrip('*') for p in params_of(header, name)[0]]


def agrees(c_type, ctype):
    """a C type ('int64_t', 'const float*') against a ctypes type: scalars by name, any pointer with any ctypes pointer type"""
    if '*' in c_type:
        return ctype in (ctypes.c_void_p, ctypes.c_char_p) or (isinstance(ctype, type) and issubclass(ctype, ctypes._Pointer))
    return ctype is SCALARS[c_type]


def check_table(ext):
    """the record's table equals its header: the same names; return type and every argument position by position; the version macro
    where the header has one; the includes the record lists and no other header of this library"""
    assert sorted(ext.table) == declared_symbols(ext.header) and ext.version_symbol in ext.table
    for name, (res, args) in ext.table.items():
        params, ret = params_of(ext.header, name)
        assert agrees(ret if '*' in ret else ret.split()[-1], res), (name, ret, res)
        assert len(params) == len(args), (name, len(params), len(args))
        for p, a in zip(params, args):
            assert agrees(p if '*' in p else p.split()[-2], a), (name, p, a)
    src = source_of(ext.header)
    if ext.version_macro:
        assert re.search(rf'#define\s+{ext.version_macro}\s+{ext.version}\s*$', src, flags=re.M), ext.version_macro
    assert re.findall(r'#include\s+"([^"]+)"', src) == list(ext.includes)
