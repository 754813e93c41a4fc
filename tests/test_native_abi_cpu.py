"""The C ABI of the kernel library is declared once, in csrc/include/cgnn_api.h, and
every file that defines or calls an entry point includes that header: the compiler then
refuses a definition whose signature drifts (extern "C" symbols link by name alone, so
nothing else would).  Plain text processing of the sources; nothing is compiled."""
import glob
import os
import re

import pytest

import cgnn_amd

CSRC = os.path.join(os.path.dirname(os.path.abspath(cgnn_amd.__file__)), "csrc")
HEADER = os.path.join(CSRC, "include", "cgnn_api.h")
SOURCES = sorted(glob.glob(os.path.join(CSRC, "kernels", "*")))
EXTERN_C = re.compile(r'extern\s+"C"\s*')


def _code(path):
    """The file's text without comments."""
    with open(path) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def _after_parameters(text, pos):
    """(function name, first character after its parameter list) of the function whose
    declarator starts at pos."""
    m = re.compile(r"[^;{}()]*?(\w+)\s*\(").match(text, pos)
    assert m, text[pos:pos + 80]
    depth, k = 1, m.end()
    while depth:
        depth += {"(": 1, ")": -1}.get(text[k], 0)
        k += 1
    return m.group(1), text[k:].lstrip()[:1]


def _extern_c(path):
    """(names defined, names only declared, extern "C" blocks) in one source file."""
    text = _code(path)
    defined, declared, blocks = [], [], 0
    for m in EXTERN_C.finditer(text):
        if text[m.end()] == "{":
            blocks += 1
            continue
        name, nxt = _after_parameters(text, m.end())
        (defined if nxt == "{" else declared).append(name)
    return defined, declared, blocks


def _header_names():
    text = _code(HEADER)
    m = EXTERN_C.search(text)
    assert m and text[m.end()] == "{", "cgnn_api.h: one extern \"C\" { ... } block"
    body = text[m.end() + 1:text.rindex("}")]
    names = []
    for decl in body.split(";")[:-1]:
        name, nxt = _after_parameters(decl + ";", 0)
        assert nxt == ";", decl
        names.append(name)
    return names


def _includes_header(path):
    return re.search(r'^\s*#\s*include\s+"cgnn_api\.h"', _code(path), re.M) is not None


def test_sources_are_found():
    assert os.path.isfile(HEADER)
    assert sum(p.endswith(".hip") for p in SOURCES) >= 12
    assert any(p.endswith("bindings.cpp") for p in SOURCES)


def test_header_declares_each_entry_point_exactly_once():
    declared = _header_names()
    assert len(declared) == len(set(declared)), sorted(n for n in declared if declared.count(n) > 1)
    defined = [n for p in SOURCES for n in _extern_c(p)[0]]
    assert len(defined) > 50 and "gnn_launch_spmm" in defined     # the parser sees the library
    assert len(defined) == len(set(defined))
    assert set(defined) - set(declared) == set(), "defined extern \"C\" but not declared in cgnn_api.h"
    assert set(declared) - set(defined) == set(), "declared in cgnn_api.h but defined nowhere"


@pytest.mark.parametrize("path", SOURCES, ids=os.path.basename)
def test_source_uses_the_header_and_declares_nothing_itself(path):
    defined, declared, blocks = _extern_c(path)
    assert declared == [] and blocks == 0, "extern \"C\" declarations belong in cgnn_api.h"
    if defined or path.endswith("bindings.cpp"):
        assert _includes_header(path), "defines or calls the C ABI without including cgnn_api.h"


def test_the_parser_tells_definitions_from_declarations(tmp_path):
    p = tmp_path / "x.hip"
    p.write_text('// extern "C" int in_a_comment(int);\n'
                 'extern "C" int defined_here(int a,\n    void (*cb)(int)) {\n  return a;\n}\n'
                 'extern "C" long only_declared(int);\n'
                 'extern "C" {\nint in_a_block(void);\n}\n')
    assert _extern_c(str(p)) == (["defined_here"], ["only_declared"], 1)
    assert not _includes_header(str(p))
