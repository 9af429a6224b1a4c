"""CPU checks of the declared boundary, once for every record of ``_lib.EXTENSIONS``: the record's table equals its header
(tests/abi_headers.check_table), the built library exports every declared symbol and its version function returns the record's value,
and no name belongs to two records.  An eleventh header needs no edit here.  No GPU, no compute calls."""
import ctypes

import pytest

import abi_headers as H
from conftest import load_pkg

EXTENSIONS = load_pkg()._lib.EXTENSIONS
each_extension = pytest.mark.parametrize('ext', EXTENSIONS, ids=[e.key for e in EXTENSIONS])


@each_extension
def test_header_equals_the_table(ext):
    H.check_table(ext)


@each_extension
def test_symbols_are_exported_and_version(ext):
    h = ctypes.CDLL(load_pkg().build.build())
    syms = H.declared_symbols(ext.header)
    assert syms
    for s in syms:
        assert hasattr(h, s), f'{s} declared in include/{ext.header} but not exported'
    assert getattr(h, ext.version_symbol)() == ext.version


def test_every_name_belongs_to_one_record():
    """no name is in two tables and no header declares a name of another record's table, in either direction"""
    L = load_pkg()._lib
    for field in ('key', 'header', 'version_symbol'):
        assert len({getattr(e, field) for e in EXTENSIONS}) == len(EXTENSIONS), field
    tables = [getattr(L, n) for n in dir(L) if n.endswith('SIGNATURES')]
    assert len(tables) == len(EXTENSIONS) and all(any(e.table is t for e in EXTENSIONS) for t in tables), 'a table without a record'
    owner = {}
    for e in EXTENSIONS:
        for name in e.table:
            assert name not in owner, f'{name} is in the tables of {owner[name]} and {e.key}'
            owner[name] = e.key
    for e in EXTENSIONS:
        for name in H.declared_symbols(e.header):
            assert owner.get(name) == e.key, f'include/{e.header} declares {name}, a name of the {owner.get(name)} table'
