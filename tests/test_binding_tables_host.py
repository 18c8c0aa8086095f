"""The binding tables of score_amd/bindings.py against the headers they bind: every declaration of a header is in its table
with as many arguments, pointers where the header has pointers and the scalar types the header names.  Host only: the
tables are bound against a stub, no library is loaded."""
import ctypes as C
import os
import re

import pytest

from score_amd.bindings import TABLES, bind

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
SCALARS = {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "double": C.c_double}
# what each header's "missing from the library" error says after "rebuild it"
MISSING = {
    "robust": "(the oracle's CPU twin has no robust loop: engine='python' runs there)",
    "refine_robust": "(the CPU twin of the tests has no robust refinement: engine='python' runs there)",
    "refine_batch": None,  # (this header's binder never had a check of its own: ctypes' AttributeError names the symbol)
    "refine_robust_batch": "(the CPU twin of the tests has no robust refinement: engine='python' runs there)",
    "marginals": "(the oracle's CPU twin has no marginals: engine='python' runs there)",
    "marginals_batch": "(the oracle's CPU twin has no marginals: engine='python' runs there)",
    "spectrum": "(the oracle's CPU twin has no eigensolver: engine='python' runs there)",
    "spectrum_batch": "(the oracle's CPU twin has no eigensolver: engine='python' runs there)",
    "samples": "(the CPU twin has no posterior samples: engine='python' runs there)",
    "samples_batch": "(the CPU twin has no posterior samples: engine='python' runs there)",
    "leverage": "(the CPU twin has no leverages: engine='python' runs there)",
}


def _declarations(name):
    """{symbol: [parameter, ...]} of include/score_<name>.h, comments stripped."""
    with open(os.path.join(INCLUDE, f"score_{name}.h")) as f:
        text = f.read()
    text = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    return {m.group(1): [" ".join(p.split()) for p in m.group(2).split(",")]
            for m in re.finditer(r"\b(score_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", text)}


class _Function:
    argtypes = restype = None


class _Stub:
    """A library whose symbols spring into being, except ``lacks``."""

    def __init__(self, lacks=None):
        self._lacks = lacks

    def __getattr__(self, name):
        if name.startswith("_") or name == self._lacks:
            raise AttributeError(name)
        fn = _Function()
        setattr(self, name, fn)
        return fn


def test_one_table_per_header():
    assert sorted(t.name for t in TABLES) == sorted(MISSING)
    assert sum(len(t) for t in TABLES) == 22


@pytest.mark.parametrize("table", TABLES, ids=lambda t: t.name)
def test_table_matches_header(table):
    declared = _declarations(table.name)
    assert sorted(declared) == sorted(table)
    lib = bind(_Stub(), table)
    assert bind(lib, table) is lib  # (bound once)
    for sym, params in declared.items():
        argtypes = getattr(lib, sym).argtypes
        assert argtypes == table[sym][0] and getattr(lib, sym).restype == table[sym][1]
        assert len(params) == len(argtypes), sym
        for param, typ in zip(params, argtypes):
            is_pointer = typ is C.c_void_p or hasattr(typ, "contents")
            assert ("*" in param) == is_pointer, (sym, param, typ)
            if not is_pointer:
                assert SCALARS[param.split()[-2]] is typ, (sym, param, typ)


@pytest.mark.parametrize("table", TABLES, ids=lambda t: t.name)
def test_missing_symbol(table):
    sym = list(table)[-1]
    if MISSING[table.name] is None:
        with pytest.raises(AttributeError, match=sym):
            bind(_Stub(lacks=sym), table)
        return
    with pytest.raises(RuntimeError) as e:
        bind(_Stub(lacks=sym), table)
    assert str(e.value) == f"{sym} is missing from the library: rebuild it {MISSING[table.name]}"
